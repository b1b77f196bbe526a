"""extractSlices over intervals of device volumes, the host side: mvsim_tile_interval, mvsim_interval_out_dim and csrc/interval_plan.h
(compiled by plain g++ under ASan + UBSan and run as a child process).  No GPU, no compute calls.

SWEEP is the case list tests/test_intervals.py runs on the GPU: (volume (Nx, Ny, Nz), min, max), inclusive corners, x first."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from . import poisson_sweep_cases as S

VOL_A = (37, 29, 23)          # Nx != Ny, odd row pitch
VOL_B = (64, 32, 16)
SWEEP = (
    ("whole", VOL_A, (0, 0, 0), (36, 28, 22)),
    ("voxel", VOL_A, (36, 28, 22), (36, 28, 22)),
    ("tx1", VOL_A, (5, 0, 0), (5, 28, 22)),
    ("tx3ty1", VOL_A, (7, 4, 0), (9, 4, 22)),             # a plane smaller than a Philox group
    ("31x26x21", VOL_A, (3, 2, 1), (33, 27, 21)),
    ("tx32", VOL_A, (4, 0, 0), (35, 28, 22)),
    ("rows", VOL_B, (0, 0, 2), (63, 31, 13)),             # whole rows and planes
)
INCS = (1, 3, 4)
SNRS = (-1.0, 0.0, 8.0, 25.0)
FAR = ((2048, 2048, 512), (2048 - 174, 2048 - 173, 512 - 58), (2047, 2047, 511))     # the far corner: byte offsets beyond 2^32, the last voxel at 2^31 - 1
K_INTERVAL = 5


def _i64(v):
    return (C.c_int64 * len(v))(*[int(x) for x in v])


def _tile(mvs, dim, ratio, tile):
    return mvs.tile_interval(dim, ratio, tile)


def test_tile_interval_restates_the_reference(mvs):
    r = (0.2, 0.2, 0.2)
    mn, mx, ov = _tile(mvs, (289,) * 3, r, 0)
    assert ov == [29] * 3 and mn == [0] * 3 and mx == [173] * 3
    mn, mx, ov = _tile(mvs, (289,) * 3, r, 1)
    assert ov == [29] * 3 and mn == [115] * 3 and mx == [288] * 3
    # 288: round(28.8) = 29, tiles of 174 and 173 voxels per side
    mn0, mx0, _ = _tile(mvs, (288,) * 3, r, 0)
    mn1, mx1, _ = _tile(mvs, (288,) * 3, r, 1)
    assert [b - a + 1 for a, b in zip(mn0, mx0)] == [174] * 3 and [b - a + 1 for a, b in zip(mn1, mx1)] == [173] * 3
    # tile 1 starts at dimension(0) / 2 - overlap_d in EVERY dimension (SimulateTileStitching.java:231), not at dim_d / 2 - overlap_d
    dim = (64, 48, 32)
    mn, mx, ov = _tile(mvs, dim, r, 1)
    assert ov == [6, 5, 3]
    assert mn == [dim[0] // 2 - o for o in ov] == [26, 27, 29] and mn != [26, 19, 13]
    assert mx == [63, 47, 31] and all(a <= b for a, b in zip(mn, mx))
    mn, mx, _ = _tile(mvs, dim, r, 0)
    assert mn == [0, 0, 0] and mx == [38, 29, 19]
    with pytest.raises(ValueError):
        _tile(mvs, dim, r, 2)


def test_tile_interval_mirror_agrees(mvs):
    """The mirror's getInterval arithmetic (unchanged) and the library's, over odd, even and non-cubic sizes and several ratios."""
    for dim in ((289,) * 3, (288,) * 3, (64, 48, 32), (33, 70, 5), (2, 2, 2)):
        for ratio in ((0.2,) * 3, (0.1, 0.25, 0.5), (0.05, 0.3, 0.0)):
            ov = [int(np.floor(dim[d] * ratio[d] / 2 + 0.5)) for d in range(3)]
            for tile in (0, 1):
                mn, mx, got = _tile(mvs, dim, ratio, tile)
                lo, hi = [0, 0, 0], [d - 1 for d in dim]
                if tile == 0:
                    hi = [dim[d] // 2 + ov[d] for d in range(3)]
                else:
                    lo = [dim[0] // 2 - ov[d] for d in range(3)]
                assert (mn, mx, got) == (lo, hi, ov), (dim, ratio, tile)


def _out_dim(mvs, dim, mn, mx, inc):
    L = mvs._lib.load()
    od = (C.c_int64 * 3)()
    job = mvs.interval_job(0x1000, dim, mn, mx, inc, -1.0)
    mvs._lib.check(L.mvsim_interval_out_dim(C.byref(job), od))
    return list(od)


def test_interval_out_dim(mvs):
    for _, dim, mn, mx in SWEEP:
        t = [b - a + 1 for a, b in zip(mn, mx)]
        for inc in INCS + (2, 7, 23, 100):
            assert _out_dim(mvs, dim, mn, mx, inc) == [t[0], t[1], (t[2] - 1) // inc + 1]
    # (tz - 1) % inc != 0: the trailing planes are not acquired
    assert _out_dim(mvs, VOL_A, (0, 0, 0), (36, 28, 22), 4) == [37, 29, 6] and (23 - 1) % 4 != 0
    assert _out_dim(mvs, VOL_A, (0, 0, 1), (36, 28, 21), 3) == [37, 29, 7] and (21 - 1) % 3 != 0
    assert _out_dim(mvs, *FAR, 3) == [174, 173, 20]
    L = mvs._lib.load()
    od = (C.c_int64 * 3)()
    assert L.mvsim_interval_out_dim(None, od) == mvs._lib.MVSIM_EINVAL
    for dim, mn, mx, inc in ((VOL_A, (0, 0, 0), (36, 28, 22), 0), (VOL_A, (3, 0, 0), (2, 28, 22), 1), (VOL_A, (0, 0, 0), (37, 28, 22), 1),
                             (VOL_A, (0, -1, 0), (36, 28, 22), 1), (VOL_A, (0, 0, 0), (36, 28, 23), 1), ((0, 4, 4), (0, 0, 0), (0, 0, 0), 1)):
        with pytest.raises(ValueError):
            _out_dim(mvs, dim, mn, mx, inc)


def test_full_overlap_on_an_even_size_leaves_the_volume(mvs):
    """Ratio 1.0: overlap = dim / 2, tile 0 = [0, dim]: one voxel past the end.  The extract calls validate as mvsim_interval_out_dim does
    (api.cpp: interval_jobs_check); tests/test_intervals.py holds them to it on the GPU."""
    mn, mx, ov = _tile(mvs, (64,) * 3, (1.0,) * 3, 0)
    assert ov == [32] * 3 and mx == [64] * 3
    with pytest.raises(ValueError, match="leaves the volume"):
        _out_dim(mvs, (64,) * 3, mn, mx, 3)


def _plan_exe(mvs, tmp_path):
    exe = str(tmp_path / "interval_plan_main")
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-Wextra", "-Werror", "-I" + os.path.join(os.path.dirname(os.path.abspath(mvs.__file__)), "csrc"),
           os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_abi", "interval_plan_main.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    return exe


def _bits(snr):
    return struct.unpack("<I", struct.pack("<f", snr))[0]


def test_plan_header_geometry_validation_and_offsets(mvs, tmp_path):
    """tests/c_abi/interval_plan_main.cpp: csrc/interval_plan.h compiled by plain g++ under ASan + UBSan (no HIP, no libmvsim.so; a child
    process, nothing preloaded).  Every sweep shape at every inc, sampled (shares 16 and 1, and no queue) and copied: the tile, the
    pitches and the 64-bit offset of its min corner restated here; the sampler form is expect_path's on the ZERO-MIN tile (never a
    vector form: aligned16 = 0), blocks and items per segment mvsim_extract_path's.  The far corner of 2048 x 2048 x 512.  Every
    interval the C ABI refuses.  The tile arithmetic against the library.  Which jobs share launches."""
    exe = _plan_exe(mvs, tmp_path)
    L = mvs._lib.load()
    geoms = []
    for _, dim, mn, mx in SWEEP + (("far",) + FAR,):
        for inc in INCS:
            for noise, share in ((1, 16), (1, 1), (1, 0), (0, 16)):
                geoms.append((dim, mn, mx, inc, noise, share))
    refused = [(VOL_A, (0, 0, 0), (36, 28, 22), 0), (VOL_A, (3, 0, 0), (2, 28, 22), 1), (VOL_A, (0, 5, 0), (36, 4, 22), 1),
               (VOL_A, (0, 0, 9), (36, 28, 8), 1), (VOL_A, (0, 0, 0), (37, 28, 22), 1), (VOL_A, (0, 0, 0), (36, 29, 22), 1),
               (VOL_A, (0, 0, 0), (36, 28, 23), 1), (VOL_A, (-1, 0, 0), (36, 28, 22), 1), ((64,) * 3, (0, 0, 0), (64, 64, 64), 3),
               ((0, 1, 1), (0, 0, 0), (0, 0, 0), 1), ((65535 * 4 + 1, 1, 1), (0, 0, 0), (0, 0, 0), 1)]
    tiles = [((289,) * 3, (0.2,) * 3), ((288,) * 3, (0.2,) * 3), ((64, 48, 32), (0.2,) * 3), ((64,) * 3, (1.0,) * 3), ((33, 70, 5), (0.1, 0.25, 0.5))]
    same = [((174, 174, 174, 3, 1, _bits(8.0)), (174, 174, 174, 3, 1, _bits(8.0)), 1), ((174, 174, 174, 3, 1, _bits(8.0)), (174, 174, 174, 3, 1, _bits(25.0)), 0),
            ((174, 174, 174, 3, 1, _bits(8.0)), (174, 173, 174, 3, 1, _bits(8.0)), 0), ((174, 174, 174, 3, 1, _bits(8.0)), (174, 174, 174, 4, 1, _bits(8.0)), 0),
            ((174, 174, 174, 3, 0, _bits(-1.0)), (174, 174, 174, 3, 0, _bits(-2.0)), 1), ((174, 174, 174, 3, 0, _bits(-1.0)), (174, 174, 174, 3, 1, _bits(0.0)), 0)]
    requests = [f"geom {d[0]} {d[1]} {d[2]} {a[0]} {a[1]} {a[2]} {b[0]} {b[1]} {b[2]} {inc} {noise} {share}" for d, a, b, inc, noise, share in geoms]
    requests += [f"geom {d[0]} {d[1]} {d[2]} {a[0]} {a[1]} {a[2]} {b[0]} {b[1]} {b[2]} {inc} 1 16" for d, a, b, inc in refused]
    requests += [f"tile {d[0]} {d[1]} {d[2]} {r[0]!r} {r[1]!r} {r[2]!r} {t}" for d, r in tiles for t in (0, 1)]
    requests += ["same " + " ".join(str(v) for v in a + b) for a, b, _ in same]
    r = subprocess.run([exe], input="\n".join(requests) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and f"interval plan run ok: {len(requests)} requests" in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    rows = [tuple(int(t) for t in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(requests)
    it = iter(rows)
    for dim, mn, mx, inc, noise, share in geoms:
        row = next(it)
        t = [b - a + 1 for a, b in zip(mn, mx)]
        nzo = (t[2] - 1) // inc + 1
        offset = mn[0] + dim[0] * (mn[1] + dim[1] * mn[2])
        assert row[:9] == (1, t[0], t[1], t[2], nzo, t[0] * t[1] * nzo, dim[0], dim[0] * dim[1], offset), (dim, mn, mx, inc)
        eff = share if noise else 0
        kernel, refuses = S.expect_path(t, inc, 0, 0, 0, eff)
        assert kernel in (S.K_NOISE2_ANY, S.K_SCALAR) and (kernel == S.K_NOISE2_ANY) == (eff != 0)
        path = (C.c_int64 * 4)()
        mvs._lib.check(L.mvsim_extract_path(_i64(t), inc, 0, 0, 0, eff, path))
        assert row[9:13] == (kernel, int(refuses), path[2], path[3]) and path[0] == kernel, (dim, mn, mx, inc, noise, share, row)
        if kernel == S.K_NOISE2_ANY:
            plane = t[0] * t[1]
            assert row[13] == ((plane + 3) // 4 + 1 + 63) // 64 and row[12] > 0 and row[14] >= row[11] * row[12] * 16
    far_offset = FAR[1][0] + 2048 * (FAR[1][1] + 2048 * FAR[1][2])
    assert 4 * far_offset > 2 ** 32 and any(row[8] == far_offset for row in rows[:len(geoms)])
    for _ in refused:
        assert next(it) == (0,)
    for dim, ratio in tiles:
        for t in (0, 1):
            mn, mx, ov = _tile(mvs, dim, ratio, t)
            assert next(it) == tuple(mn + mx + ov), (dim, ratio, t)
    for a, b, want in same:
        assert next(it) == (want,), (a, b)


def test_ctypes_job_matches_the_header_struct(mvs):
    """mvsim_interval_job as include/mvsim.h lays it out on this ABI: pointer, 9 x int64, int32, float, uint64, uint32 (+ padding)."""
    J = mvs.IntervalJob
    assert C.sizeof(J) == 104
    assert [getattr(J, f).offset for f in ("in_", "dim", "min", "max", "inc", "snr", "seed", "stream")] == [0, 8, 32, 56, 80, 84, 88, 96]
