"""Deterministic cases of the stacked-view sweep (tests/test_stacked_views_sweep.py): mvsim_simulate_views_dev with the views STACKED
(csrc/api_view.cpp: views_enqueue_batched) over every kernel form that call reaches -- the LDS-table rotate + attenuate kernel with the
view table at every row length it takes another shape for, passes A, B, D and E on V x Nz planes of every tile form, the direct z pass
with the view in its grid (k_zconv and k_zconv_strided<2|3|4>, one and several chunks per column, the strided pitch), the view counts and
the sampler behind them.  Pure Python: the CPU tests check the landings, the coverage and the yardstick's sensitivity from the same list
the GPU tests run.

Shapes are (x, y, z) here, as the library and conv_sweep_cases count them; numpy volumes are (z, y, x).

One target of the issue does not exist: nkxb == 1.  nkxb = hxp / 16 and hxp is M + 1 rounded up to 16 or more columns, where M >= 16 is
the x half length (the shortest entry of the size table): hxp >= 32 and nkxb >= 2 for every volume.  The sweep takes nkxb == 2, the
smallest there is, and nkxb > 2 (test_the_smallest_column_group_count_is_two holds the library to that)."""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field

from .conv_sweep_cases import MAX_MACS, NLZ, hxp, lines_per_tile, pick, pick_x, split_taken

MAX_VIEWS = 32                      # MVSIM_MAX_VIEWS
GEO_CHUNK = 512                     # rows per geometry table of k_rotate_attenuate_axis0_lds (rotate.hip)
ROT_BLOCK = 1024                    # columns per block of that kernel: 16 waves
SEED = 464232194

# the targets of the sweep; every one is named by exactly one case, and that case's own shape lands on it (landing)
TARGETS = (
    # rotate + attenuate with the view table
    "nx17", "nx130", "nx640", "nx>1024", "ny>nx", "nz1", "nz5", "nz8", "nz9", "angles",
    # y and x lengths with V * Nz planes
    "y16", "y8", "ysplit", "nkxb2", "nkxb>2",
    # the direct z pass
    "kz1", "kz2", "kz9", "kz31", "kz64", "kz>nz", "nch>=2", "inc1", "strided2", "strided3", "strided4", "cost-rule", "inc5", "inc7", "inc>nz",
    "inc2-zconv_strided0", "inc2-exp2",
    # view count, extract
    "V2", "V3", "V8", "V32", "plane%4",
)
ANGLES_STACK = (0, 33, 90, 120, 180, -52, -90, 120)        # 0, 90, 180, -90, 33, -52 and two views of one angle, never adjacent


@dataclass
class Case:
    name: str
    dim: tuple                 # (Nx, Ny, Nz)
    kdim: tuple                # (Kx, Ky, Kz)
    degrees: tuple             # one angle per view
    targets: tuple             # what this case is in the sweep for
    inc: int = 1
    opts: dict = field(default_factory=dict)     # convolution options, set in the stacked and in the sequential context alike

    @property
    def id(self) -> str:
        o = "".join(f"-{k}={v}" for k, v in self.opts.items())
        return f"{self.name}-{'x'.join(map(str, self.dim))}-k{'x'.join(map(str, self.kdim))}-inc{self.inc}-V{self.V}{o}"

    @property
    def V(self) -> int:
        return len(self.degrees)

    @property
    def shape(self):           # numpy (z, y, x)
        return self.dim[::-1]

    @property
    def kshape(self):
        return self.kdim[::-1]

    @property
    def macs(self) -> int:
        """Multiply-adds of the fp64 direct sum of ONE view."""
        return self.dim[0] * self.dim[1] * self.dim[2] * self.kdim[0] * self.kdim[1] * self.kdim[2]

    @property
    def nzo(self) -> int:
        return (self.dim[2] - 1) // self.inc + 1

    def seed(self, v: int) -> int:
        return SEED + 7919 * v + zlib.crc32(self.name.encode()) % 1000

    def stream(self, v: int) -> int:
        return 3 * v + 1

    def padded(self):
        """(Px, Py) and the row pitch of the spectrum (the direct z pass: every case has Kz <= 64)."""
        px, py = 2 * pick_x(self.dim[0] + self.kdim[0] - 1), pick(self.dim[1] + self.kdim[1] - 1)
        return px, py, hxp(px, py, 16, True)


def _spread(n: int, step: int = 37, first: int = -170):
    """n different whole angles in (-180, 180), neighbours `step` degrees apart."""
    out = [(first + 180 + step * v) % 360 - 180 for v in range(n)]
    assert len(set(out)) == n
    return tuple(out)


def cases():
    """Every case of the sweep, in a fixed order: the smallest shapes that still reach each form."""
    return [
        # ---- the rotate kernel: one partial wave; inactive lanes in the third wave; two geometry chunks; two x blocks; Ny > Nx
        Case("nx17", (17, 17, 5), (2, 3, 9), (25, -140), ("nx17", "nz5", "kz>nz", "V2", "plane%4")),
        Case("nx130", (130, 130, 1), (3, 2, 2), (0, 2, -3), ("nx130", "nz1", "kz2", "V3")),
        Case("nx640", (640, 640, 2), (3, 3, 3), (0, 177), ("nx640", "y8", "nkxb>2")),
        Case("nx1030", (1030, 1030, 2), (2, 2, 2), (180, -4), ("nx>1024",)),
        Case("tall", (20, 45, 8), (3, 4, 1), (40, -15, 160), ("ny>nx", "nz8", "kz1", "y16", "nkxb2")),
        Case("angles", (20, 24, 9), (3, 4, 9), ANGLES_STACK, ("angles", "nz9", "kz9", "V8", "inc1")),
        # ---- y lines split into two half-length transforms
        Case("ysplit", (64, 2010, 2), (3, 31, 2), (0, 180), ("ysplit",)),
        # ---- the direct z pass: the deepest PSF; two chunks per column; the three strided instances with nzp > Nz; what keeps k_zconv
        # on the strided pitch -- the cost rule, inc >= 5, inc > Nz (one plane per view), the option -- and the rule overridden
        Case("kz64", (18, 20, 70), (2, 3, 64), (50, -75), ("kz64",)),
        Case("chunks", (16, 16, 270), (3, 3, 31), (12, -160), ("nch>=2", "kz31")),
        Case("inc2", (20, 22, 37), (3, 3, 15), (35, -80, 160), ("strided2",), inc=2),
        Case("inc3", (20, 22, 38), (2, 3, 17), (35, -80, 160), ("strided3",), inc=3),
        Case("inc4", (20, 22, 41), (3, 2, 16), (35, -80, 160), ("strided4",), inc=4),
        Case("refused", (20, 22, 37), (3, 3, 7), (35, -80, 160), ("cost-rule",), inc=2),
        Case("inc5", (20, 22, 13), (3, 3, 5), (35, -80, 160), ("inc5",), inc=5),
        Case("inc7", (20, 22, 16), (3, 3, 4), (35, -80, 160), ("inc7",), inc=7),
        Case("inc11", (20, 22, 6), (3, 3, 3), (35, -80, 160), ("inc>nz",), inc=11),
        Case("plain", (20, 22, 37), (3, 3, 15), (35, -80, 160), ("inc2-zconv_strided0",), inc=2, opts={"zconv_strided": 0}),
        Case("forced", (20, 22, 37), (3, 3, 7), (35, -80, 160), ("inc2-exp2",), inc=2, opts={"exp": 2}),
        # ---- as many views as one call takes
        Case("most", (16, 18, 4), (2, 2, 3), _spread(MAX_VIEWS), ("V32",)),
    ]


def landing(c: Case) -> set:
    """Every target the case's own shape lands on -- computed from the shape, not from what the case claims.  The z kernel, zc and nch
    are the library's to say (mvsim_zpass_geometry, asserted beside this in the CPU test): `zgeo` targets are listed by zpass_targets."""
    nx, ny, nz = c.dim
    kx, ky, kz = c.kdim
    px, py, pitch = c.padded()
    out = set()
    waves = min((nx + 63) // 64, 16)
    if nx == 17:
        assert waves == 1                                        # one partial wave
        out.add("nx17")
    if nx == 130:
        assert waves == 3 and nx % 64 == 2
        out.add("nx130")
    if GEO_CHUNK < nx <= ROT_BLOCK and nx == 640:
        assert (nx + GEO_CHUNK - 1) // GEO_CHUNK == 2 and (nx + waves * 64 - 1) // (waves * 64) == 1
        out.add("nx640")
    if nx > ROT_BLOCK:
        assert (nx + waves * 64 - 1) // (waves * 64) == 2
        out.add("nx>1024")
    if ny > nx:
        out.add("ny>nx")
    if nz in (1, 5, 8, 9):
        out.add(f"nz{nz}")
    if c.degrees == ANGLES_STACK:
        out.add("angles")
    if lines_per_tile(py) == 16:
        out.add("y16")
    if 640 <= py <= 1920:
        assert lines_per_tile(py) == 8
        out.add("y8")
    if py == 2048 and split_taken(c.dim, c.kdim, exp=c.opts.get("exp", 0)):
        out.add("ysplit")
    out.add("nkxb2" if pitch // NLZ == 2 else "nkxb>2")
    if kz in (1, 2, 9, 31, 64):
        out.add(f"kz{kz}")
    if kz > nz:
        out.add("kz>nz")
    out.add(f"V{c.V}")
    if (nx * ny) % 4:
        out.add("plane%4")
    return out


def zpass_targets(c: Case, zgeo) -> set:
    """The z pass targets a case lands on, given the library's (kernel, zc, nch, nkxb) for its geometry under the DEFAULT options."""
    kernel, _, nch, _ = zgeo
    nz, inc = c.dim[2], c.inc
    strided_on = c.opts.get("zconv_strided", 1) != 0
    forced = bool(c.opts.get("exp", 0) & 2)
    out = set()
    if nch >= 2:
        out.add("nch>=2")
    if inc == 1:
        assert kernel == 0
        out.add("inc1")
    elif 2 <= inc <= 4 and nz % inc:
        assert c.nzo * inc > nz                                  # the strided pitch is longer than the view
        if not strided_on:
            assert kernel == inc                                 # ... the option is what keeps k_zconv
            out.add(f"inc{inc}-zconv_strided0")
        elif forced:
            assert kernel == 0                                   # ... the cost rule would have refused
            out.add(f"inc{inc}-exp2")
        elif kernel == inc:
            out.add(f"strided{inc}")
        else:
            assert kernel == 0
            out.add("cost-rule")
    elif inc > nz:
        assert kernel == 0 and c.nzo == 1
        out.add("inc>nz")
    elif inc in (5, 7):
        assert kernel == 0 and c.nzo * inc > nz
        out.add(f"inc{inc}")
    return out


__all__ = ["Case", "cases", "landing", "zpass_targets", "TARGETS", "ANGLES_STACK", "MAX_VIEWS", "MAX_MACS", "SEED"]
