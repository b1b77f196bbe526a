"""Deterministic case list of the extract + Poisson sweep (tests/test_poisson_sweep.py): pure Python, no GPU, no library.

Every case names an entry point, a geometry, a queue setting, an RNG key and counter range, and the sampler form it claims to
land on; `launch_args` restates the geometry the entry point hands the extract stage (extract_plan.h: ExtractGeom, as mvsim_extract_path's
arguments), and `expect_path` restates the decision that extract_plan makes on it.  The CPU tests hold both to the library; the GPU tests run the cases."""
import math
from dataclasses import dataclass, field

import numpy as np

SEED = 464232194
SEED_BOTH = 0x9E3779B97F4A7C15          # both 32-bit words of the Philox key non-zero
SEED_MAX = 2 ** 64 - 1
STREAMS = (0, 5, 2 ** 32 - 1)
KEYS = (SEED, SEED_BOTH, SEED_MAX)

# kernels of mvsim_extract_path; FUSED: the fused tail of the convolution's last pass (mvsim_fused_tail_geometry)
K_SCALAR, K_VEC, K_NOISE2, K_NOISE2_ANY, FUSED = 0, 1, 2, 3, 4
QUEUES = ("16", "1", "auto", "off")
# counter boundaries a wave straddles: the sign bit of the index's low word (a signed 32-bit widening), the low word of the index, of
# the pair block (index >> 1), of the group block (index >> 2), and the sign bit of a signed 64-bit cast
BOUNDARIES = (2 ** 31, 2 ** 32, 2 ** 33, 2 ** 34, 2 ** 63)
# plane sizes (ny, nx): 4, 12, 60, 255, 256, 257, 61 x 63, 64 x 64 and 1020 voxels
PLANES = ((1, 4), (3, 4), (6, 10), (15, 17), (16, 16), (1, 257), (63, 61), (64, 64), (30, 34))
INCS = (1, 2, 3, 7)
SNR_UNIT = math.sqrt(5.0)               # poisson_process: mul = (snr / sqrt 5)^2 = 1 exactly, so lambda = v (exactly 10.0 exists)
SNR = 25.0                              # float SNR of extractSlices and the views: mul = 124.99999999999997

ENTRIES = ("poisson", "extract", "extract_dev", "view", "view_con", "view_fused", "views", "slab3", "slab_dev")
VIEW_ENTRIES = ("view", "view_con", "view_fused", "views", "slab3", "slab_dev")


@dataclass(frozen=True)
class Case:
    id: str
    entry: str
    shape: tuple                 # (nz, ny, nx) of the input volume; poisson: (1, 1, n)
    inc: int = 1
    queue: str = "16"
    seed: int = SEED
    stream: int = 0
    offset: int = 0              # poisson_process: index_offset
    slab: tuple = ()             # slab cases: (z0, z1)
    claim: int = K_NOISE2        # the kernel the case lands on
    refuses: bool = False        # its queue segments can refuse voxels (share < 16): refused walk 1 or 2
    adjust: bool = False
    views: int = 1
    tags: tuple = field(default_factory=tuple)

    @property
    def plane(self):
        return self.shape[1] * self.shape[2]


def mul_of(case):
    """Tools.poissonProcess's lambda / value (Tools.java:76) as the entry point computes it."""
    if case.entry == "poisson":
        return (SNR_UNIT / math.sqrt(5.0)) ** 2
    s = float(np.float32(SNR))
    return (s / math.sqrt(5.0)) ** 2


def share_of(queue, total):
    """What share_for (extract_plan.h) resolves the option to: auto gives small queues (<= 4 Mi voxels) every voxel."""
    if queue == "off":
        return 0
    if queue == "auto":
        assert total <= 4 << 20
        return 16
    return int(queue)


def acquired(nz, inc):
    return (nz - 1) // inc + 1


def slab_planes(case):
    """(first acquired source plane, acquired planes, compact?) of a slab case (extract_plan.h: ExtractGeom::slab; api_view.cpp: slab_finish_enqueue)."""
    z0, z1 = case.slab
    k0, k1 = (z0 + case.inc - 1) // case.inc, (z1 + case.inc - 1) // case.inc
    return k0 * case.inc, k1 - k0, case.inc > 1 and z0 % case.inc == 0


def launch_args(case):
    """(dim, inc, index_inc, index_offset, aligned16, queue share) of the launch_extract call the entry point makes."""
    nz, ny, nx = case.shape
    plane = nx * ny
    nzo = acquired(nz, case.inc)
    on = case.queue != "off"
    if case.entry == "poisson":
        n = case.shape[2]
        return (n, 1, 1), 1, 0, case.offset, 1, share_of(case.queue, n)
    if case.entry in ("extract", "extract_dev"):
        return (nx, ny, nz), case.inc, 0, 0, 0 if case.entry == "extract_dev" else 1, share_of(case.queue, plane * nzo)
    share = share_of(case.queue, plane * nzo)
    if case.entry in ("view", "views"):
        # an untiled view convolves only the acquired planes (compact) when the queue samples them (api_view.cpp: view_enqueue)
        if case.inc > 1 and on:
            return (nx, ny, nzo), 1, case.inc, 0, 1, share
        return (nx, ny, nz), case.inc, 0, 0, 1, share
    if case.entry == "view_con":
        return (nx, ny, nz), case.inc, 0, 0, 1, share
    if case.entry in ("slab3", "slab_dev"):
        z0, z1 = case.slab
        first, n_acq, compact = slab_planes(case)
        share = share_of(case.queue, plane * n_acq)
        if compact:
            return (nx, ny, n_acq), 1, case.inc, z0 * plane, 1, share
        return (nx, ny, z1 - first), case.inc, 0, first * plane, int(plane * (first - z0) % 4 == 0), share
    raise ValueError(case.entry)


def expect_path(dim, inc, index_inc, offset, aligned16, share):
    """(kernel, segments can refuse) restated from extract_plan (extract_plan.h)."""
    if index_inc <= 0:
        index_inc = inc
    plane = dim[0] * dim[1]
    total = plane * acquired(dim[2], inc)
    crossings = -(-255 // plane)
    queue = share != 0 and crossings * (index_inc - 1) * plane < 2 ** 31 and total < 2 ** 32 and plane < 2 ** 32
    vec = plane % 4 == 0 and offset % 4 == 0 and aligned16
    if queue:
        return (K_NOISE2 if vec else K_NOISE2_ANY), share < 16
    return (K_VEC if vec else K_SCALAR), False


def lambda_mix(n, mul, seed, exact_ten=False):
    """A fixed mix of values v (lambda = (double) v * mul) over n voxels: zero, negative, NaN, 1e-30, the background (1e-4), the
    inversion regime, the low-lambda shortcut's edge (lambda ~ 1), phase 1's class edges (9.99 / 10.01), exactly 10.0 (mul = 1 only)
    and its float neighbours, PTRS up to 1e6, one run above 1e9 (no squeeze) up to 1e15, and dark holes inside bright pairs."""
    rng = np.random.default_rng(seed)
    lam = np.empty(n, np.float64)
    cat = rng.choice(12, size=n, p=[.03, .02, .02, .02, .06, .30, .06, .04, .04, .30, .01, .10])
    lam[cat == 0] = 0.0
    lam[cat == 1] = -rng.random((cat == 1).sum()) * 5 - 1e-3
    lam[cat == 2] = np.nan
    lam[cat == 3] = 1e-30 * mul
    lam[cat == 4] = 1e-4 * mul
    lam[cat == 5] = rng.uniform(0.01, 9.9, (cat == 5).sum())
    lam[cat == 6] = rng.uniform(0.97, 1.03, (cat == 6).sum())
    lam[cat == 7] = rng.choice([9.99, 10.01, 9.9899, 10.0101], (cat == 7).sum())
    lam[cat == 8] = 10.0
    lam[cat == 9] = np.exp(rng.uniform(np.log(10.0), np.log(1e6), (cat == 9).sum()))
    lam[cat == 10] = np.exp(rng.uniform(np.log(1.1e9), np.log(1e15), (cat == 10).sum()))
    # holes: a bright pair with one dark member (phase 1 compacts PAIRS of voxels)
    holes = np.flatnonzero(cat == 11)
    lam[holes] = np.where(holes % 2 == 0, np.exp(rng.uniform(np.log(10.0), np.log(1e4), holes.size)), 0.0)
    v = (lam / mul).astype(np.float32)
    if exact_ten:
        ten = np.float32(10.0 / mul)
        assert float(ten) * mul == 10.0
        v[cat == 8] = ten
        # just either side of 10
        s = np.flatnonzero(cat == 8)
        v[s[0::3]] = np.nextafter(ten, np.float32(0))
        v[s[1::3]] = np.nextafter(ten, np.float32(np.inf))
    return v


def _poisson_cases():
    out = []
    i = 0
    # each counter boundary inside one wave, vector (offset = B - 128, n % 4 == 0) and group-by-group (offset = B - 127 or B - 125,
    # or n % 4 != 0) forms, queue on and off
    for b in BOUNDARIES:
        for form, off, n in (("vec", b - 128, 8192), ("any", b - 127, 8192), ("any3", b - 125, 8190), ("anyn", b - 256, 8191)):
            for q in ("16", "off") if form in ("vec", "any") else ("1",) if form == "any3" else ("auto",):
                key = KEYS[i % 3]
                st = STREAMS[(i // 3) % 3]
                args = ((n, 1, 1), 1, 0, off, 1, share_of(q, n))
                k, r = expect_path(*args)
                out.append(Case(f"poisson-{form}-b{b.bit_length() - 1}-q{q}", "poisson", (1, 1, n), queue=q, seed=key, stream=st,
                                offset=off, claim=k, refuses=r, tags=(f"boundary{b.bit_length() - 1}",)))
                i += 1
    # offsets 0 and 1, 2, 3 (mod 4) next to an aligned one, small counters
    for off, q in ((0, "16"), (0, "1"), (1002, "16"), (1001, "1"), (1003, "off"), (1000, "off")):
        args = ((16384, 1, 1), 1, 0, off, 1, share_of(q, 16384))
        k, r = expect_path(*args)
        out.append(Case(f"poisson-off{off}-q{q}", "poisson", (1, 1, 16384), queue=q, seed=KEYS[i % 3], stream=STREAMS[i % 3],
                        offset=off, claim=k, refuses=r))
        i += 1
    return out


def _extract_cases():
    out = []
    i = 0
    for gi, (ny, nx) in enumerate(PLANES):
        plane = ny * nx
        for entry in ("extract", "extract_dev"):
            inc = INCS[(gi + (entry == "extract_dev")) % 4]
            q = QUEUES[(gi + 2 * (entry == "extract_dev")) % 4]
            nzo = max(3, -(-4096 // plane))
            nz = (nzo - 1) * inc + 1 + (inc - 1) // 2          # trailing planes extractSlices does not read
            c = Case(f"{entry}-{ny}x{nx}-inc{inc}-q{q}", entry, (nz, ny, nx), inc=inc, queue=q, seed=KEYS[i % 3],
                     stream=STREAMS[(i + 1) % 3])
            k, r = expect_path(*launch_args(c))
            out.append(Case(c.id, entry, c.shape, inc=inc, queue=q, seed=c.seed, stream=c.stream, claim=k, refuses=r))
            i += 1
    return out


def _view_cases():
    spec = [
        # entry, (nz, ny, nx), inc, queue, seed, stream, slab
        ("view", (24, 64, 64), 3, "16", SEED_BOTH, 5, ()),
        ("view", (20, 63, 61), 2, "1", SEED, 2 ** 32 - 1, ()),
        ("view", (22, 64, 64), 3, "off", SEED_MAX, 0, ()),
        ("view", (22, 63, 61), 7, "off", SEED_BOTH, 5, ()),
        ("view", (18, 64, 64), 1, "auto", SEED, 5, ()),
        ("view_con", (20, 64, 64), 2, "auto", SEED_MAX, 5, ()),
        ("view_con", (21, 63, 61), 3, "16", SEED_BOTH, 0, ()),
        ("view_con", (20, 63, 61), 2, "1", SEED, 5, ()),
        ("view_fused", (24, 64, 64), 3, "16", SEED_BOTH, 2 ** 32 - 1, ()),
        ("views", (20, 64, 64), 2, "16", SEED, 5, ()),
        ("views", (21, 63, 61), 3, "1", SEED_BOTH, 0, ()),
        ("views", (20, 64, 64), 1, "1", SEED_MAX, 5, ()),
        ("views", (20, 63, 61), 2, "16", SEED_MAX, 2 ** 32 - 1, ()),
        ("slab3", (32, 64, 64), 3, "16", SEED_BOTH, 5, (0, 16)),
        ("slab3", (32, 64, 64), 3, "1", SEED, 0, (16, 32)),
        ("slab3", (28, 63, 61), 2, "16", SEED_MAX, 5, (13, 28)),
        ("slab_dev", (28, 63, 61), 2, "1", SEED_BOTH, 2 ** 32 - 1, (0, 14)),
        ("slab_dev", (32, 64, 64), 3, "auto", SEED, 5, (17, 32)),
        ("slab_dev", (30, 64, 64), 3, "16", SEED_MAX, 0, (0, 15)),
    ]
    out = []
    for entry, shape, inc, q, seed, st, slab in spec:
        ident = f"{entry}-{shape[1]}x{shape[2]}x{shape[0]}-inc{inc}-q{q}" + (f"-z{slab[0]}_{slab[1]}" if slab else "")
        c = Case(ident, entry, shape, inc=inc, queue=q, seed=seed, stream=st, slab=slab, views=3 if entry == "views" else 1)
        if entry == "view_fused":
            k, r = FUSED, False
        else:
            k, r = expect_path(*launch_args(c))
        out.append(Case(c.id, entry, shape, inc=inc, queue=q, seed=seed, stream=st, slab=slab, claim=k, refuses=r,
                        adjust=entry != "view_con", views=c.views))
    return out


CASES = _poisson_cases() + _extract_cases() + _view_cases()


def counters_of(case):
    """[(first counter of acquired plane k)] for the extract / view / slab cases: source plane (z0 +) k * inc, global index."""
    nz, ny, nx = case.shape
    plane = nx * ny
    if case.entry in ("slab3", "slab_dev"):
        first, n_acq, _ = slab_planes(case)
        return [(first + k * case.inc) * plane for k in range(n_acq)]
    return [k * case.inc * plane for k in range(acquired(nz, case.inc))]
