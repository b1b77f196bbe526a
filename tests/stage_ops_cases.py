"""Deterministic cases of the stage-operator sweep (tests/test_stage_ops_sweep.py): sum / adjust / norm, makeIsotropic, the weight
image, the cross-view weight normalisation, downSample2x and the bead normalisation, each at the sizes where its launcher changes
form (16-byte body or scalar), leaves a tail behind the body, or runs into its block cap and becomes a grid-stride loop.

The module restates every launcher's form predicate and block cap as constants and small functions; the CPU tests hold them to
the launchers' source and decide the coverage from them.  Inputs are seeded from crc32(case.id).  Shapes are numpy's (nz, ny, nx)."""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

THREADS = 256
# block caps of the launchers (kernels.hip, common.h, phantom.hip, beads.hip)
ISO_BX_CAP = 64              # launch_make_isotropic: blocks along a plane; one output plane per blockIdx.y
ISO_MAX_PLANES = 65535       # ... and the output planes one launch takes
WEIGHT_IMAGE_CAP = 8192      # launch_weight_image
SUM_BLOCKS = 2048            # launch_sum (k_sum_partial)
ADJUST_CAP = 4096            # launch_adjust_apply
NORM_CAP = 4096              # launch_norm_apply
WEIGHTS_CAP = 8192           # launch_weights
DOWNSAMPLE_CAP = 16384       # launch_downsample2x
BEADS_MINMAX_CAP = 1024      # beads_normalize_dev: k_minmax (NORM_BLOCKS)
BEADS_APPLY_CAP = 8192       # ... and its k_norm_apply
MAX_VIEWS = 32               # MVSIM_MAX_VIEWS
COSINE_SPAN = 40             # computeWeightImage's ramp
OSEM = 3.0


def _want(items: int) -> int:
    return (items + THREADS - 1) // THREADS


# ---------------------------------------------------------------------------------------- form predicates and caps, restated
def iso_vec(plane: int, aligned: bool) -> bool:
    """launch_make_isotropic takes k_make_isotropic<true>: plane % 4 == 0 and both pointers 16-byte aligned."""
    return plane % 4 == 0 and aligned


def iso_items(plane: int, aligned: bool) -> int:
    """Loop items per plane: float4s in the vector form, voxels in the scalar one."""
    return plane // 4 if iso_vec(plane, aligned) else plane


def iso_above(plane: int, aligned: bool) -> bool:
    return _want(iso_items(plane, aligned)) > ISO_BX_CAP


def sum_vec(aligned: bool) -> bool:
    """k_sum_partial and k_adjust_apply: n >> 2 float4s when the pointer is 16-byte aligned, else none (all in the scalar loop)."""
    return aligned


def sum_blocks(n: int) -> int:
    return min(max((n // 4 + 255) // 256, 1), SUM_BLOCKS)


def sum_above(n: int) -> bool:
    return (n // 4 + 255) // 256 > SUM_BLOCKS


def adjust_above(n: int) -> bool:
    return (n // 4 + 255) // 256 > ADJUST_CAP


def norm_above(n: int) -> bool:
    return _want(n) > NORM_CAP


def sum_depth(n: int, aligned: bool = True) -> int:
    """R: the number of additions on the longest path from one voxel to the result of k_sum_partial + k_sum_final, read off the
    kernels.  Thread 0 of block 0 has the most trips.  In k_sum_partial a voxel of the first float4 goes through 2 additions of
    ((x + y) + (z + w)) and then one `acc +=` per float4 trip (T4) and per scalar trip (Ts); wave_sum adds 6, the block's
    ((s0 + s1) + (s2 + s3)) 2.  k_sum_final: one `acc +=` per partial of the thread (F = ceil(blocks / 256)), then 6 + 2 again."""
    blocks = sum_blocks(n)
    nthreads = blocks * THREADS
    n4 = n >> 2 if sum_vec(aligned) else 0
    t4 = -(-n4 // nthreads)
    ts = -(-(n - 4 * n4) // nthreads)
    return (2 + t4 if t4 else 0) + ts + 8 + -(-blocks // 256) + 8


# ---------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    op: str                    # iso | weight | adjust | norm | weights | down | beads
    shape: tuple = ()          # (nz, ny, nx) of the input (weight image: of the output)
    inc: int = 0               # iso
    n: int = 0                 # adjust, norm, beads: voxels; weights: voxels per view
    views: int = 0             # weights
    kind: str = "uniform"      # input kind: uniform | mixed | desc | zeros ; beads: where the extremes are planted
    offset: bool = False       # through the _dev entry point on pointers 4 bytes past a 16-byte boundary
    refused: bool = False      # the launcher must refuse it (ValueError)
    R: int = 0                 # adjust, norm: sum_depth(n, aligned), written out

    @property
    def id(self) -> str:
        dims = "x".join(str(s) for s in self.shape) if self.shape else f"n{self.n}"
        parts = [self.op, dims]
        if self.inc:
            parts.append(f"inc{self.inc}")
        if self.views:
            parts.append(f"v{self.views}")
        if self.kind != "uniform":
            parts.append(self.kind)
        if self.offset:
            parts.append("off4")
        if self.refused:
            parts.append("refused")
        return "-".join(parts)

    @property
    def aligned(self) -> bool:
        return not self.offset

    @property
    def plane(self) -> int:
        return self.shape[1] * self.shape[2]

    @property
    def seed(self) -> int:
        return zlib.crc32(self.id.encode())


SUM_SIZES = (1, 3, 4, 5, 1023, 4097,
             2097152 + 4099,       # past the SUM_BLOCKS cap, tail of 3
             2097152 + 4100,       # ... without a tail
             4194304 + 3,          # the last size the adjust cap still holds in one trip (4096 blocks exactly), tail of 3
             4194304 + 7,          # past the adjust cap: thread 0 takes a second float4; tail of 3
             4194304 + 8)          # ... without a tail
# R per size for the aligned form (test_sum_depths_are_the_written_ones holds them to sum_depth)
SUM_R = {1: 18, 3: 18, 4: 20, 5: 21, 1023: 21, 4097: 21, 2101251: 29, 2101252: 28, 4194307: 29, 4194311: 30, 4194312: 29,
         1048577: 24, 1048580: 24}
SUM_R_UNALIGNED = {4099: 22, 4100: 21, 2101251: 29}
NORM_SIZES = (1, 3, 4, 5, 1023, 4097, 1048576 + 1, 1048576 + 4)


def _iso_cases():
    out = []
    for inc in (1, 3, 4, 7):
        out.append(Case("iso", (5, 8, 12), inc=inc))                          # vector, small: 24 float4s per plane
        out.append(Case("iso", (5, 7, 9), inc=inc))                           # scalar, small: 63 voxels per plane
    out += [
        Case("iso", (3, 32, 32), inc=2),                                      # vector, one full block per plane
        Case("iso", (2, 256, 260), inc=2),                                    # vector across the cap: 65 blocks wanted, whole blocks
        Case("iso", (2, 257, 260), inc=2),                                    # ... with a partly filled last block
        Case("iso", (2, 127, 130), inc=2),                                    # scalar across the cap: 16 510 voxels per plane
        Case("iso", (1, 4, 4), inc=5),                                        # nz == 1: one output plane, mirror1's n == 1
        Case("iso", (2, 4, 4), inc=3),                                        # nz == 2: the mirror period is 2
        Case("iso", (2, 1, 1), inc=65534),                                    # 65 535 output planes: the last accepted count
        Case("iso", (2, 1, 1), inc=65535, refused=True),                      # 65 536
        Case("iso", (3, 8, 12), inc=3, offset=True),                          # vector-sized plane, unaligned pointers: scalar form
        Case("iso", (3, 16, 16), inc=2, offset=True),                         # ... scalar form with whole blocks
        Case("iso", (2, 128, 130), inc=2, offset=True),                       # ... across the cap with whole blocks
        Case("iso", (3, 8, 12), inc=3, kind="mixed"),                         # mixed signs, and a -0.0 in the last plane
    ]
    return out


def _weight_cases():
    out = [Case("weight", (2, ny, 3)) for ny in (1, 2, 39, 40, 41, 80, 81, 82, 100, 101)]
    out += [
        Case("weight", (2, 64, 2)),                                           # one whole block
        Case("weight", (33, 256, 250)),                                       # 8250 blocks wanted: above the cap, whole blocks
        Case("weight", (33, 255, 251)),                                       # ... with a partly filled last block
        Case("weight", (2, 101, 3), offset=True),
    ]
    return out


def _sum_cases():
    out = []
    for n in SUM_SIZES:
        out.append(Case("adjust", n=n, R=SUM_R[n]))
        out.append(Case("adjust", n=n, kind="desc", R=SUM_R[n]))
    for n in (1, 5, 4097):
        out.append(Case("adjust", n=n, kind="zeros", R=SUM_R[n]))
    for n in sorted(SUM_R_UNALIGNED):                                         # adjust_image_dev on dptr + 4: n4 = 0 in both kernels
        out.append(Case("adjust", n=n, kind="desc", offset=True, R=SUM_R_UNALIGNED[n]))
    for n in NORM_SIZES:
        out.append(Case("norm", n=n, R=SUM_R[n]))
        out.append(Case("norm", n=n, kind="desc", R=SUM_R[n]))
    return out


def _weights_cases():
    out = [Case("weights", n=n, views=v) for v in (1, 2, 7, 32) for n in (1, 255, 1920)]
    out += [Case("weights", n=256, views=4),
            Case("weights", n=2097152 + 513, views=2),                        # above the cap
            Case("weights", n=2097152 + 512, views=2)]                        # ... with whole blocks
    return out


def _down_cases():
    return [Case("down", s) for s in ((4, 4, 4),          # one output voxel
                                      (9, 8, 21), (10, 13, 16), (5, 6, 7), (12, 7, 4), (18, 18, 34))]      # the last: 1024 outputs, whole blocks


BEADS_PLANTS = ("min_last", "max_last", "min_first", "max_first")


def _beads_cases():
    out = [Case("beads", n=1, kind="none")]
    for n in (2, 255, 256, 257, 262144 + 3, 262144 + 256, 2097152 + 5):       # past k_minmax's cap, and past k_norm_apply's
        out += [Case("beads", n=n, kind="min_last"), Case("beads", n=n, kind="max_last")]
    for n in (257, 262144 + 3):
        out += [Case("beads", n=n, kind="min_first"), Case("beads", n=n, kind="max_first")]
    return out


def cases(op: str | None = None):
    allc = _iso_cases() + _weight_cases() + _sum_cases() + _weights_cases() + _down_cases() + _beads_cases()
    return [c for c in allc if op is None or c.op == op]


# ---------------------------------------------------------------------------------------- inputs
WEIGHT_PATTERNS = ("all_zero", "plus_minus", "neg_zero", "cancel4", "dominant")


def weight_plants(case: Case) -> dict:
    """pattern -> voxel index for a weights case: whichever patterns its view count can hold, spread over the image and ending on
    its last voxel; a one-voxel case holds one pattern, chosen by its seed."""
    ok = [p for p in WEIGHT_PATTERNS if case.views >= {"plus_minus": 2, "cancel4": 4}.get(p, 1)]
    if case.n < len(ok):
        ok = ok[case.seed % len(ok):][:case.n]
    return {p: ((k + 1) * case.n) // len(ok) - 1 for k, p in enumerate(ok)}


def inputs(case: Case):
    """The case's input: one float32 array, or the list of views for a weights case.  A fresh copy on every call."""
    rng = np.random.default_rng(case.seed)
    if case.op in ("iso", "down"):
        if case.kind == "mixed":
            v = (rng.random(case.shape, dtype=np.float32) - np.float32(0.5)) * np.float32(2)
            # The z + 1 tap of the last output plane has weight 0 and lands on the mirrored plane nz - 2; all it can decide is the sign
            # of a zero.  A -0.0 with negative x / y neighbours and a positive voxel below it: -0 + (+v * 0) = +0 with the right mirror.
            v[-1, 2:4, 3:5] = -np.abs(v[-1, 2:4, 3:5]) - np.float32(0.25)
            v[-1, 2, 3] = np.float32(-0.0)
            v[-2, 2:4, 3:5] = np.abs(v[-2, 2:4, 3:5]) + np.float32(0.25)
            return v
        return rng.random(case.shape, dtype=np.float32)
    if case.op in ("adjust", "norm"):
        if case.kind == "zeros":
            return np.zeros(case.n, np.float32)
        if case.kind == "desc":
            # positive, 2^20 of dynamic range, largest first: a float or a back-to-front accumulation loses the small end
            return np.sort(np.exp2(-20.0 * rng.random(case.n)).astype(np.float32))[::-1].copy()
        return rng.random(case.n, dtype=np.float32) * np.float32(2)
    if case.op == "weights":
        ws = [np.ascontiguousarray(rng.random(case.n, dtype=np.float32) * (rng.random(case.n) > 0.3), dtype=np.float32)
              for _ in range(case.views)]
        for name, i in weight_plants(case).items():
            col = np.zeros(case.views, np.float32)
            if name == "plus_minus":
                col[:2] = (0.75, -0.75)
            elif name == "neg_zero":
                col[:] = -0.0
            elif name == "cancel4":
                col[:4] = (1e8, 1.0, -1e8, 1.0)       # float sum in view order 1, back to front 0, in double 2
            elif name == "dominant":
                col[:] = 0.125
                col[case.views - 1] = 5.0             # osem * 5 / sum > 1: clamped
            for v in range(case.views):
                ws[v][i] = col[v]
        return ws
    if case.op == "beads":
        x = (rng.random(case.n, dtype=np.float32) - np.float32(0.5)) * np.float32(200)
        if case.kind != "none":
            what, where = case.kind.split("_")
            x[-1 if where == "last" else 0] = np.float32(-1000.0 if what == "min" else 1000.0)
        return x
    raise ValueError(case.op)
