"""A literal restatement of the procedural phantom's arithmetic, independent of the package: its own
java.util.Random, fdlibm logarithm and nextGaussian(), the Perlin constructor and value, the brute-force sphere value, the sequential
rejection sampler and the sequence of HypersphereCollectionRealRandomAccessible.main.  Element-wise numpy fp64 / float32 operations
are IEEE-exact (one rounding each); ``np.fmod`` on float32 stands for Java's float ``%``."""
import math
import struct

import numpy as np

MASK = (1 << 48) - 1
MULT = 0x5DEECE66D


class Lcg:
    """java.util.Random from the JDK specification."""

    def __init__(self, seed=None, state=None):
        self.s = ((seed ^ MULT) & MASK) if state is None else state
        self.pending = None

    def next(self, bits):
        self.s = (self.s * MULT + 0xB) & MASK
        v = self.s >> (48 - bits)
        return v - (1 << 32) if v & 0x80000000 else v

    def next_int(self, bound):
        r = self.next(31)
        m = bound - 1
        if bound & m == 0:
            return (bound * r) >> 31
        u = r
        while True:
            r = u % bound
            if u - r + m < (1 << 31):                  # no int overflow
                return r
            u = self.next(31)

    def next_double(self):
        return ((self.next(26) << 27) + self.next(27)) * (1.0 / (1 << 53))

    def next_gaussian(self):
        if self.pending is not None:
            g, self.pending = self.pending, None
            return g
        while True:
            v1 = 2 * self.next_double() - 1
            v2 = 2 * self.next_double() - 1
            s = v1 * v1 + v2 * v2
            if not (s >= 1 or s == 0):
                break
        multiplier = math.sqrt(-2 * fdlibm_log(s) / s)
        self.pending = v2 * multiplier
        return v1 * multiplier


def _d(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


LN2_HI, LN2_LO, TWO54 = _d(0x3fe62e42fee00000), _d(0x3dea39ef35793c76), _d(0x4350000000000000)
LG = [_d(b) for b in (0x3FE5555555555593, 0x3FD999999997FA04, 0x3FD2492494229359, 0x3FCC71C51D8E78AF, 0x3FC7466496CB03DE,
                      0x3FC39A09D078C69F, 0x3FC2F112DF3E5244)]


def fdlibm_log(x):
    """__ieee754_log of fdlibm's e_log.c (StrictMath.log), line by line, for x > 0 finite (all nextGaussian() passes)."""
    assert x > 0 and math.isfinite(x)
    b = _bits(x)
    hx, k = b >> 32, 0
    if hx < 0x00100000:
        k -= 54
        x *= TWO54
        b = _bits(x)
        hx = b >> 32
    k += (hx >> 20) - 1023
    hx &= 0x000fffff
    i = (hx + 0x95f64) & 0x100000
    x = _d(((hx | (i ^ 0x3ff00000)) << 32) | (b & 0xffffffff))
    k += i >> 20
    f = x - 1.0
    dk = float(k)
    if (0x000fffff & (2 + hx)) < 3:
        if f == 0.0:
            return 0.0 if k == 0 else dk * LN2_HI + dk * LN2_LO
        R = f * f * (0.5 - 0.33333333333333333 * f)
        return f - R if k == 0 else dk * LN2_HI - ((R - dk * LN2_LO) - f)
    s = f / (2.0 + f)
    z = s * s
    i = hx - 0x6147a
    w = z * z
    j = 0x6b851 - hx
    t1 = w * (LG[1] + w * (LG[3] + w * LG[5]))
    t2 = z * (LG[0] + w * (LG[2] + w * (LG[4] + w * LG[6])))
    i |= j
    R = t2 + t1
    if i > 0:
        hfsq = 0.5 * f * f
        if k == 0:
            return f - (hfsq - s * (hfsq + R))
        return dk * LN2_HI - ((hfsq - (s * (hfsq + R) + dk * LN2_LO)) - f)
    if k == 0:
        return f - s * (f - R)
    return dk * LN2_HI - ((s * (f - R) - dk * LN2_LO) - f)


def shuffle(lst, rnd):
    """Collections.shuffle(list, rnd)."""
    i = len(lst)
    while i > 1:
        j = rnd.next_int(i)
        lst[i - 1], lst[j] = lst[j], lst[i - 1]
        i -= 1


def perlin_init(n_vectors, rnd):
    """The constructor (Perlin:56-73): gradients (n, 3) and the permutation."""
    grad = np.empty((n_vectors, 3), dtype=np.float64)
    for i in range(n_vectors):
        res, s_sum = [0.0, 0.0, 0.0], 0.0
        for d in range(3):
            res[d] = rnd.next_gaussian()
            s_sum += res[d] * res[d]
        for d in range(3):
            res[d] /= math.sqrt(s_sum)
        grad[i] = res
    perm = list(range(n_vectors))
    shuffle(perm, rnd)
    return grad, np.array(perm, dtype=np.int32)


def _smoothstep(a1, a2, p, use_pow):
    if use_pow:
        sstep = np.power(p, 3.0) * (10 - 15 * p + 6 * np.power(p, 2.0))
    else:
        sstep = (p * p * p) * (10 - 15 * p + 6 * (p * p))
    sstep = np.minimum(1.0, np.maximum(sstep, 0.0))
    return (1.0 - sstep) * a1 + sstep * a2


def perlin_value(pos, scales, extents, grad, perm, use_pow=False):
    """PerlinNoiseRealRandomAccess.get() (:127-160) at (n, 3) positions -> n doubles."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n_vectors = len(perm)
    pg, pi = [], []
    for d in range(3):
        a = (pos[:, d] / np.float64(scales[d])).astype(np.float32)
        b = np.float32(extents[d])
        mod = np.fmod(a, b)
        assert mod.dtype == np.float32
        mod = np.where(mod < 0, (mod + b).astype(np.float32), mod)
        pg.append(mod.astype(np.float64))
        pi.append(np.floor(pg[d]).astype(np.int64))
    dots, offs = [], None
    for i in range(8):
        off = (i // 4, (i % 4) // 2, i % 2)
        dist, idx, cp = [], 0, 1
        for d in range(3):
            npos = pi[d] + off[d]
            dist.append(pg[d] - npos.astype(np.float64))
            npos = npos % extents[d]
            idx = idx + npos * cp
            cp += cp * extents[d]
        if offs is None:
            offs = dist
        g = grad[perm[idx % n_vectors]]
        dot = np.zeros(len(pos), dtype=np.float64)
        for d in range(3):
            dot = dot + g[:, d] * dist[d]
        dots.append(dot)
    inter = dots
    for d in (2, 1, 0):
        inter = [_smoothstep(inter[2 * i], inter[2 * i + 1], offs[d], use_pow) for i in range(2 ** d)]
    return inter[0]


def perlin_field(pos, scales, extents, grad, perm, threshold=None):
    """What the readers of the field see: the raw value, or SimpleCalculated's lambda (:221-223) over the FloatType the value is
    stored in: (float)value > threshold ? 1 : 0."""
    v = perlin_value(pos, scales, extents, grad, perm)
    if threshold is None:
        return v
    return np.where(v.astype(np.float32).astype(np.float64) > threshold, 1.0, 0.0)


def grid_positions(dim, origin=(0, 0, 0)):
    """The integer positions of a raster, x fastest, as (n, 3) doubles."""
    z, y, x = np.meshgrid(*(np.arange(origin[d], origin[d] + dim[d], dtype=np.float64) for d in (2, 1, 0)), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)


def spheres_value(pos, centres, radii, values, background=0.0):
    """The value of the lowest-index sphere with sqrt(dx dx + dy dy + dz dz) <= radius (squares summed x, y, z), else background."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    out = np.full(len(pos), np.float32(background), dtype=np.float32)
    free = np.ones(len(pos), dtype=bool)
    for c, r, v in zip(np.asarray(centres, dtype=np.float64).reshape(-1, 3), radii, values):
        dist = np.zeros(len(pos))
        for d in range(3):
            q = pos[:, d] - c[d]
            dist = dist + q * q
        hit = free & (np.sqrt(dist) <= r)
        out[hit] = np.float32(v)
        free &= ~hit
    return out


def sample_points(rmin, rmax, n_samples, density, rnd):
    """PointRejectionSampling.sampleRealPoints (:37-55), sequentially; density(pos (3,)) -> the FloatType's value as a double.
    Returns (points (n, 3), trials)."""
    out, trials = [], 0
    while len(out) < n_samples:
        pos = [rmin[d] + rnd.next_double() * (rmax[d] - rmin[d]) for d in range(3)]
        p = rnd.next_double()
        trials += 1
        if p < density(pos):
            out.append(pos)
    return np.array(out, dtype=np.float64).reshape(-1, 3), trials


def perlin_density(scales, extents, grad, perm, threshold=None):
    def f(pos):
        v = perlin_field(pos, scales, extents, grad, perm, threshold)[0]
        return float(np.float32(v))
    return f


def spheres_density(centres, radii, values, background=0.0):
    def f(pos):
        return float(spheres_value(pos, centres, radii, values, background)[0])
    return f


def phantom_main(dim, seed=42, n_big=400, n_small=20000):
    """HypersphereCollectionRealRandomAccessible.main (:201-280) with the reference's constants: the volume (Nz, Ny, Nx)."""
    rnd = Lcg(seed)
    f32 = np.float32
    scales = (float(dim[0] // 4), dim[1] / 1.5, float(dim[2]))
    ext = (15, 15, 15)
    grad, perm = perlin_init(100, rnd)
    rmin, rmax = (0.0, 0.0, 0.0), tuple(float(d - 1) for d in dim)
    big_pos, _ = sample_points(rmin, rmax, n_big, perlin_density(scales, ext, grad, perm, 0.1), rnd)
    big_r = [float(f32(20)) + rnd.next_double() * float(f32(40) - f32(20)) for _ in range(n_big)]
    small_pos, _ = sample_points(rmin, rmax, n_small, spheres_density(big_pos, big_r, [1.0] * n_big), rnd)
    small_r, small_v = [], []
    for _ in range(n_small):
        small_r.append(float(f32(2)) + rnd.next_double() * float(f32(4) - f32(2)))
        small_v.append(f32(float(f32(4.0)) + rnd.next_double() * float(f32(6.0) - f32(4.0))))
    big_v = [f32(float(f32(1.2)) + rnd.next_double() * float(f32(2.4) - f32(1.2))) for _ in range(n_big)]
    pos = grid_positions(dim)
    res = np.zeros(len(pos), dtype=np.float32)
    res = np.maximum(res, spheres_value(pos, big_pos, big_r, big_v))
    res = np.maximum(res, spheres_value(pos, small_pos, small_r, small_v))
    return res.reshape(dim[2], dim[1], dim[0]), rnd.s
