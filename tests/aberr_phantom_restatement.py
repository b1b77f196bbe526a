"""The phantom of the refraction simulator restated in Python from the semantics of SimulateMultiViewAberrations.simulate(rnd, dir)
(:408-440) and multiSpheres (:474-586): one sequential java.util.Random, ImgLib2 HyperSphere geometry (nested truncated radii, x
fastest), float stores through setReal.  Independent of the package under test: its own generator, its own sphere walk.  Small volumes
only -- every voxel of the large sphere is one round of a Python loop."""
import math

import numpy as np

MASK = (1 << 48) - 1
MUL = 0x5DEECE66D
ADD = 0xB


def scramble(seed: int) -> int:
    """the state right after new Random(seed)"""
    return (seed ^ MUL) & MASK


def jump(state: int, k: int) -> int:
    """the state after k steps"""
    a_k, c_k, a, c = 1, 0, MUL, ADD
    while k:
        if k & 1:
            a_k, c_k = (a_k * a) & MASK, (c_k * a + c) & MASK
        c = ((a + 1) * c) & MASK
        a = (a * a) & MASK
        k >>= 1
    return (state * a_k + c_k) & MASK


class Rnd:
    """java.util.Random by the JDK's specification, counting its steps."""

    def __init__(self, state: int):
        self.s = state & MASK
        self.steps = 0

    def next(self, bits: int) -> int:
        self.s = (self.s * MUL + ADD) & MASK
        self.steps += 1
        return self.s >> (48 - bits)                  # bits <= 31: never negative as an int

    def nextInt(self, bound: int) -> int:
        r = self.next(31)
        m = bound - 1
        if bound & m == 0:
            return (bound * r) >> 31
        u = r
        while True:
            r = u % bound
            if u - r + m < (1 << 31):                 # no overflow of the int sum
                return r
            u = self.next(31)

    def nextDouble(self) -> float:
        return ((self.next(26) << 27) + self.next(27)) * (1.0 / (1 << 53))


def sphere_rows(radius: int):
    """(dz, dy, r0) of every row of a HyperSphere of this radius, in cursor order; the row holds dx = -r0 .. r0."""
    for dz in range(-radius, radius + 1):
        r1 = math.isqrt(radius * radius - dz * dz)
        for dy in range(-r1, r1 + 1):
            yield dz, dy, math.isqrt(r1 * r1 - dy * dy)


def sphere_size(radius: int) -> int:
    return sum(2 * r0 + 1 for _, _, r0 in sphere_rows(radius))


def large_radius(shape_zyx, scale: int) -> int:
    return min(shape_zyx) // 2 - 47 * scale - 1


def walk(rnd: Rnd, radius: int, scale: int, rule: str):
    """The walk over the large sphere: [(ordinal, (dx, dy, dz), raw nextInt, second double, position of the voxel's first draw, steps)]
    of the accepted voxels.  rule "draw": Math.round(rv * 10000) % (7 scale)^3 == 0; "multi": rv * 100000 < 1."""
    out = []
    modulus = (7 * scale) ** 3
    bound = 10 * scale
    ordinal = 0
    for dz, dy, r0 in sphere_rows(radius):
        for dx in range(-r0, r0 + 1):
            start = rnd.steps
            raw = rnd.nextInt(bound)
            rv = rnd.nextDouble()
            take = (math.floor(rv * 10000 + 0.5) % modulus == 0) if rule == "draw" else (rv * 100000 < 1)
            if take:
                value = rnd.nextDouble()
                out.append((ordinal, (dx, dy, dz), raw, value, start, rnd.steps - start))
            ordinal += 1
    return out


def _ball(radius: int):
    """index offsets (dz, dy, dx) of a small HyperSphere"""
    zs, ys, xs = [], [], []
    for dz, dy, r0 in sphere_rows(radius):
        for dx in range(-r0, r0 + 1):
            zs.append(dz), ys.append(dy), xs.append(dx)
    return np.array(zs), np.array(ys), np.array(xs)


def ri_noise(ri: np.ndarray, rnd: Rnd) -> None:
    """:425-426 in place: t <- (float)Math.max(0, t + (nextDouble() - 0.5) / 10), x fastest."""
    flat = ri.reshape(-1)
    for i in range(flat.size):
        v = float(flat[i]) + (rnd.nextDouble() - 0.5) / 10
        flat[i] = np.float32(v if v > 0.0 else 0.0)


def multi_spheres(img: np.ndarray, ri: np.ndarray, scale: int, rnd: Rnd):
    """:474-586 in place on (Nz, Ny, Nx) float32 volumes, sphere after sphere in the reference's order.  Returns the radii drawn."""
    nz, ny, nx = img.shape
    radius = large_radius(img.shape, scale)
    if radius < 0:
        raise ValueError("image too small")
    radii = []
    for _, (dx, dy, dz), raw, value, _, _ in walk(rnd, radius, scale, "multi"):
        r = max(raw + 1, 10 * scale - 1)
        radii.append(r)
        value_ri = value * (1.1 - 1.0) + 1.0
        value_im = value * (1.0 - 0.5) + 0.5
        bz, by, bx = _ball(r)
        z, y, x = bz + (nz // 2 + dz), by + (ny // 2 + dy), bx + (nx // 2 + dx)
        if z.min() < 0 or y.min() < 0 or x.min() < 0 or z.max() >= nz or y.max() >= ny or x.max() >= nx:
            raise ValueError("a small sphere leaves the image")
        img[z, y, x] = np.maximum(value_im, img[z, y, x].astype(np.float64)).astype(np.float32)
        old = ri[z, y, x].astype(np.float64)
        ri[z, y, x] = np.where(old == 5.0, value_ri, np.maximum(value_ri, old)).astype(np.float32)
    return radii
