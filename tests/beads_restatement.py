"""Sequential restatement of SimulateBeads.renderPoints (SimulateBeads.java:97-205) in plain numpy: the yardstick of the bead
kernels.  One bead at a time in list order, fp64 factors, float32 accumulation -- the reference's own loop order per voxel."""
import math

import numpy as np


def kernel_diameter(sigma):
    return max(3, 2 * int(3 * sigma + 0.5) + 1) if sigma > 0 else 3


def java_round(x):
    f = math.floor(x)
    return int(f) + (1 if x - f >= 0.5 else 0)


def apply(m, pts):
    m = np.asarray(m, dtype=np.float64).reshape(3, 4)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([((x * m[r, 0] + y * m[r, 1]) + z * m[r, 2]) + m[r, 3] for r in range(3)], axis=1)


def beads_in(points, interval):
    """isInsideAdjust over the list: the adjusted locations of the beads that are kept, in order."""
    mn, mx = interval
    kept = []
    for p in np.asarray(points, dtype=np.float64):
        q = [float(p[0]), float(p[1]), float(p[2])]
        ok = True
        for d in range(3):
            q[d] -= float(mn[d])
            if q[d] < 0 or q[d] > float(mx[d] - mn[d]):
                ok = False
                break
        if ok:
            kept.append(q)
    return kept


def render(points, interval, sigma, window=None):
    """The float image of one list ((Nz, Ny, Nx), Nd = max - min), or of the sub-box window = ((x0, y0, z0), (x1, y1, z1))
    (exclusive ends) of it.  Returns (image, number of voxel contributions)."""
    mn, mx = interval
    dim = [mx[d] - mn[d] for d in range(3)]
    w0, w1 = window if window is not None else ((0, 0, 0), tuple(dim))
    img = np.zeros((w1[2] - w0[2], w1[1] - w0[1], w1[0] - w0[0]), dtype=np.float32)
    size = [kernel_diameter(s) * 2 for s in sigma]
    tss = [2 * float(s) * float(s) for s in sigma]
    contributions = 0
    for loc in beads_in(points, interval):
        a, b = [], []
        for d in range(3):
            lo = java_round(loc[d]) - size[d] // 2
            a.append(max(lo, 0, w0[d]))
            b.append(min(lo + size[d] - 1, dim[d] - 1, w1[d] - 1))
        if any(a[d] > b[d] for d in range(3)):
            continue
        f = []
        for d in range(3):
            x = loc[d] - np.arange(a[d], b[d] + 1, dtype=np.float64)
            f.append(np.exp(-(x * x) / tss[d]))
        value = (f[0][None, None, :] * f[1][None, :, None]) * f[2][:, None, None]
        win = img[a[2] - w0[2]:b[2] + 1 - w0[2], a[1] - w0[1]:b[1] + 1 - w0[1], a[0] - w0[0]:b[0] + 1 - w0[0]]
        win[...] = win + value.astype(np.float32) * np.float32(1000.0)
        contributions += value.size
    return img, contributions
