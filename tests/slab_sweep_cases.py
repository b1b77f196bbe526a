"""Deterministic cases of the z-slab sweep (tests/test_slab_sweep.py): one view cut into z slabs, every slab held to the untiled view.
Pure Python: the CPU tests prove the class coverage and the yardstick's sensitivity from the same list the GPU tests run.

A case is (dim, kdim, inc, cuts): the slabs are [cuts[i], cuts[i + 1]).  `nslabs` set: the cuts are mvsim_slab_range's for that many
ranks; unset: explicit cuts.  Shapes are (x, y, z) here, as the library counts them; numpy volumes are (z, y, x).

The predicates below restate the slab arithmetic of csrc/api_view.cpp and csrc/extract_plan.h (ExtractGeom::slab) in the plainest form;
test_slab_sweep holds them to brute force and to the oracle's convolution."""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

from . import conv_sweep_cases as CS

SEED = 464232194
SNRS = (-1.0, 8.0, 25.0)
DELTA = 0.01
MIN_VALUE, TARGET = 1e-4, 1.0
INCS_SWEPT = (2, 3, 4, 7)                 # spacings that need a compact and a non-compact slab each
NSLABS_SWEPT = (1, 2, 3, 5, 8)
STRIDED_INCS = (2, 3, 4)                  # spacings k_zconv_strided is instantiated for (the default-options tier)


def slab_range(nz: int, nranks: int, rank: int):
    """mvsim_slab_range."""
    return nz * rank // nranks, nz * (rank + 1) // nranks


def range_cuts(nz: int, nslabs: int):
    return tuple(nz * r // nslabs for r in range(nslabs + 1))


@dataclass(frozen=True)
class Case:
    name: str
    dim: tuple                 # (Nx, Ny, Nz)
    kdim: tuple                # (Kx, Ky, Kz)
    inc: int
    cuts: tuple                # 0 = cuts[0] < cuts[1] < ... < cuts[-1] = Nz
    nslabs: int = 0            # > 0: cuts == range_cuts(Nz, nslabs)
    degrees: int = 20
    gt_z: tuple = ()           # z ranges of the ground truth that hold anything (empty: all of it)

    @property
    def id(self) -> str:
        how = f"r{self.nslabs}" if self.nslabs else "cuts" + "_".join(map(str, self.cuts))
        return f"{self.name}-{'x'.join(map(str, self.dim))}-k{'x'.join(map(str, self.kdim))}-inc{self.inc}-{how}"

    @property
    def shape(self):           # numpy (z, y, x)
        return self.dim[::-1]

    @property
    def kshape(self):
        return self.kdim[::-1]

    @property
    def nz(self) -> int:
        return self.dim[2]

    @property
    def kz(self) -> int:
        return self.kdim[2]

    @property
    def slabs(self):
        return list(zip(self.cuts, self.cuts[1:]))

    @property
    def fused_eligible(self) -> bool:
        return CS.fused_geometry_ok(self.dim, self.kdim)


# ---------------------------------------------------------------------------------------- the slab arithmetic, restated plainly
def extract_nz(nz: int, inc: int) -> int:
    return (nz - 1) // inc + 1


def acquired(z0: int, z1: int, inc: int):
    """The acquired planes of a slab by enumeration: every k with z0 <= k * inc < z1."""
    return [k for k in range(0, z1 // inc + 2) if z0 <= k * inc < z1]


def nzo(z0: int, z1: int, inc: int) -> int:
    return len(acquired(z0, z1, inc))


def is_compact(z0: int, inc: int) -> bool:
    """The slab's buffer keeps its acquired planes alone (the library's choice with the early sum: the slab starts on a plane the view reads)."""
    return inc > 1 and z0 % inc == 0


def first_acquired_is_last_plane(z0: int, z1: int, inc: int) -> bool:
    a = acquired(z0, z1, inc)
    return bool(a) and a[0] * inc == z1 - 1


def tap_reach(kz: int):
    """(below, above): output plane z reads the input planes z - below .. z + above (centre Kz / 2, no flip)."""
    c = kz // 2
    return kz - 1 - c, c


def folds(nz: int, kz: int, z0: int, z1: int):
    """(low, high): the taps of the slab's outputs reach below plane 0 / above plane Nz - 1."""
    below, above = tap_reach(kz)
    return z0 - below < 0, z1 - 1 + above > nz - 1


def mirror(i: int, n: int) -> int:
    """The oracle's mirror rule (oracle._mirror_pad): single mirror, period 2 n - 2."""
    if n == 1:
        return 0
    p = 2 * n - 2
    i %= p
    return i if i < n else p - i


def reached_planes(nz: int, kz: int, z0: int, z1: int):
    """Every input plane a tap of an output in [z0, z1) reads, by enumeration."""
    below, above = tap_reach(kz)
    return sorted({mirror(i, nz) for z in range(z0, z1) for i in range(z - below, z + above + 1)})


def no_range_gives(cuts) -> bool:
    nz = cuts[-1]
    return all(range_cuts(nz, n) != tuple(cuts) for n in range(1, nz + 1))


def ground_truth(case: Case) -> np.ndarray:
    """Non-negative (nothing cancels in a sum), sparse, nothing outside case.gt_z."""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    gt = (rng.random(case.shape, dtype=np.float32) * (rng.random(case.shape) < 0.5)).astype(np.float32)
    if case.gt_z:
        keep = np.zeros(case.nz, bool)
        for a, b in case.gt_z:
            keep[a:b] = True
        gt[~keep] = 0.0
    return gt


def psf_of(case: Case) -> np.ndarray:
    """Not symmetric: a flipped tap order or a wrong centre is a large error."""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()) ^ 0x5AB)
    return (rng.random(case.kshape, dtype=np.float32) + 0.05).astype(np.float32)


# ---------------------------------------------------------------------------------------- cases
def _r(name, dim, kdim, inc, nslabs, **kw):
    return Case(name, dim, kdim, inc, range_cuts(dim[2], nslabs), nslabs=nslabs, **kw)


def _c(name, dim, kdim, inc, cuts, **kw):
    assert cuts[0] == 0 and cuts[-1] == dim[2] and all(a < b for a, b in zip(cuts, cuts[1:])), name
    return Case(name, dim, kdim, inc, tuple(cuts), **kw)


def cases():
    """Every case of the sweep, in a fixed order."""
    out = [
        # spacing 1; a fold at the low face only ([0, 8)) and at the high face only ([8, 16))
        _r("inc1", (12, 12, 16), (3, 3, 5), 1, 2),
        # the whole view as its only slab
        _r("one_slab", (14, 14, 11), (3, 5, 5), 3, 1, degrees=-40),
        # inc 2: starts 7 (non-compact) and 14 (compact); an even PSF depth; an odd plane size (no float4 path in the extraction)
        _r("inc2_even_kz", (13, 17, 21), (3, 5, 4), 2, 3),
        # inc 3, five unequal slabs: starts 4, 13 non-compact, 9, 18 compact; even depth
        _r("inc3_unequal", (12, 18, 23), (5, 3, 6), 3, 5, degrees=33),
        # inc 4, eight slabs of 4 or 5 planes: starts 9, 13, 18, 23, 27 non-compact, 4, 32 compact
        _r("inc4_eight", (16, 16, 37), (3, 3, 3), 4, 8),
        # inc 7: 13 and 26 non-compact; then 14 compact and 30 non-compact
        _r("inc7", (12, 14, 40), (3, 3, 9), 7, 3, degrees=50),
        _c("inc7_cuts", (12, 20, 40), (3, 4, 6), 7, (0, 14, 30, 40)),
        # [5, 7) at inc 4 acquires nothing; [7, 9) acquires plane 8 alone, its last
        _c("empty_and_last", (12, 12, 12), (3, 3, 3), 4, (0, 5, 7, 9, 12)),
        _c("empty_inc7", (16, 24, 15), (3, 3, 2), 7, (0, 8, 14, 15), degrees=90),
        # one tap along z: no halo at all
        _r("kz1", (12, 12, 9), (3, 3, 1), 2, 3),
        # 64 taps: [32, 48) reaches [1, 80) -- no fold; the slabs around it fold, all halos are deeper than their slabs
        _r("kz64", (12, 12, 80), (1, 3, 64), 3, 5, degrees=10),
        _r("kz64_even_slabs", (12, 16, 70), (3, 1, 64), 2, 2),
        # more taps than planes: every slab folds at both faces, more than once
        _r("kz_ge_nz", (12, 16, 6), (3, 3, 9), 2, 2),
        _r("kz_eq_nz", (14, 14, 4), (3, 3, 4), 3, 2, degrees=0),
        _c("kz64_thin", (12, 12, 5), (3, 3, 64), 4, (0, 1, 3, 5)),
        _r("two_planes", (12, 16, 2), (3, 3, 5), 2, 2, degrees=5),
        # a halo deeper than the slab, fewer taps than planes
        _r("deep_halo", (12, 12, 30), (3, 3, 8), 1, 5),
        _r("deep_halo_inc3", (20, 33, 31), (3, 3, 15), 3, 8, degrees=-25),
        # no fold in the middle slab
        _r("no_fold", (12, 12, 24), (3, 3, 3), 2, 3),
        # slabs one plane deep next to a deep one: cuts no slab_range produces
        _c("depth1", (12, 12, 10), (3, 3, 4), 2, (0, 1, 2, 9, 10)),
        _c("depth1_inc3", (14, 22, 13), (3, 3, 7), 3, (0, 1, 2, 12, 13), degrees=-15),
        _r("all_depth1", (12, 16, 8), (3, 3, 3), 2, 8),
        # compact starts away from plane 0, depths that are no multiple of the spacing: the strided z pass of a slab
        _c("compact2", (16, 20, 34), (3, 3, 7), 2, (0, 6, 17, 24, 34)),
        _c("compact3", (24, 40, 40), (5, 5, 10), 3, (0, 6, 16, 33, 40), degrees=40),
        _r("compact4", (16, 20, 48), (3, 3, 11), 4, 3),
        _c("compact4_cuts", (20, 28, 45), (3, 3, 31), 4, (0, 8, 21, 28, 45), degrees=-60),
        # the ground truth ends at plane 8 and the view does not turn: [16, 24) and its halo [15, 24) hold exact zeros
        _r("zero_slab", (12, 12, 24), (3, 3, 3), 2, 3, degrees=0, gt_z=((0, 8),)),
        _c("zero_slab_inc3", (12, 20, 30), (3, 3, 5), 3, (0, 7, 16, 23, 30), degrees=0, gt_z=((10, 14),)),
        # the smallest shapes the fused rotate + attenuate + x transform takes (Nx >= 64, padded half length 72)
        _r("fused_x", (126, 128, 10), (5, 3, 3), 2, 2),
        _c("fused_x_inc3", (126, 128, 12), (5, 3, 4), 3, (0, 3, 7, 12), degrees=-30),
    ]
    for c in out:
        assert c.cuts[0] == 0 and c.cuts[-1] == c.nz and (not c.nslabs or c.cuts == range_cuts(c.nz, c.nslabs)), c.id
        assert c.dim[0] <= c.dim[1] and 1 <= c.kz <= 64, c.id
    return out


# ---------------------------------------------------------------------------------------- classes the list must cover
def case_classes(case: Case):
    """The classes of the issue's list that the case as a whole decides, each by a predicate above."""
    out = set()
    nz, kz, inc = case.nz, case.kz, case.inc
    out.add("inc1" if inc == 1 else f"inc{inc}")
    out.add("kz_even" if kz % 2 == 0 else "kz_odd")
    if kz == 1:
        out.add("kz1")
    if kz == 64:
        out.add("kz64")
    if kz >= nz:
        out.add("kz_ge_nz")
    if len({z1 - z0 for z0, z1 in case.slabs}) > 1:
        out.add("unequal_depths")
    if case.nslabs:
        out.add(f"nslabs{case.nslabs}")
    elif no_range_gives(case.cuts):
        out.add("cuts_no_range_gives")
    if case.dim[1] > case.dim[0]:
        out.add("ny_gt_nx")
    if case.fused_eligible:
        out.add("fused_x")
    return out


def slab_classes(case: Case, z0: int, z1: int):
    """... and those one slab decides (the all-zero slab needs the attenuated volume: test_slab_sweep decides it with the oracle)."""
    out = set()
    nz, kz, inc = case.nz, case.kz, case.inc
    if inc > 1:
        out.add(f"inc{inc}_{'compact' if is_compact(z0, inc) else 'noncompact'}")
    if nzo(z0, z1, inc) == 0:
        out.add("nzo0")
    if first_acquired_is_last_plane(z0, z1, inc):
        out.add("first_acquired_is_last")
    if kz > z1 - z0:
        out.add("halo_deeper_than_slab")
    lo, hi = folds(nz, kz, z0, z1)
    out.add({(True, False): "fold_low_only", (False, True): "fold_high_only", (True, True): "fold_both", (False, False): "no_fold"}[(lo, hi)])
    if z1 - z0 == 1:
        out.add("depth1")
    return out


def classes_of(case: Case):
    out = case_classes(case)
    for z0, z1 in case.slabs:
        out |= slab_classes(case, z0, z1)
    return out


def required_classes():
    req = {"inc1", "kz_even", "kz_odd", "kz1", "kz64", "kz_ge_nz", "halo_deeper_than_slab", "fold_low_only", "fold_high_only", "fold_both",
           "no_fold", "depth1", "unequal_depths", "cuts_no_range_gives", "nzo0", "first_acquired_is_last", "fused_x", "ny_gt_nx"}
    req |= {f"inc{i}_{f}" for i in INCS_SWEPT for f in ("compact", "noncompact")}
    req |= {f"nslabs{n}" for n in NSLABS_SWEPT}
    return req
