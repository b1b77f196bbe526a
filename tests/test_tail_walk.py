"""The trip walk of the vector sampler behind a sparse tail (k_extract4_noise2_sparse, csrc/extract.hip; the walk: csrc/extract_plan.h).
A wave of that kernel walks the output with a grid stride of 16 384 blocks x 256 float4 groups; the flags of its trips are a bit mask
it loads before its first trip, and the plane a trip starts in is carried from trip to trip.  The GPU cases of tests/test_skip_tail.py
end after ONE trip (their largest volume is 4 096 blocks); only volumes of more than 16.8 M voxels send a wave on a second one.  These are
the smallest such shapes, one for each instance of the kernel:

  aligned      (nz, ny, nx) = (68, 512, 512): 65 536 groups per plane, a multiple of 64 -- a slot lies in one plane; blocks 0 .. 1 023
               make a second trip, into planes 64 .. 67;
  straddling   (72, 510, 508): 64 770 groups per plane, 2 mod 64 -- every plane boundary lies inside a slot; 4 663 440 groups, the second
               trip reaches planes 64 .. 71.

The specimens have non-empty planes among those of a first trip and among those of a second, and empty planes among both (PSF of three
z taps: the dilated flags reach one plane further on each side; the specimen is eight rows thin in y, so that 3 degrees about x move it
by less than a plane).  The check is that of test_skip_tail.py: skip_tail = 1 equals skip_tail = 0 and skip_empty = 0 bit for bit in
acquisition and factor, the same items were queued, mvsim_get_tail_path says the mode ran and planes were skipped."""
import os
import shutil
import subprocess

import numpy as np
import pytest

SEED = 464232195
PSF_SHAPE = (3, 5, 5)
#         name          (nz, ny, nx)      non-empty planes of the specimen
CASES = {"aligned": ((68, 512, 512), (33, 34, 64)),
         "straddling": ((72, 510, 508), (35, 36, 66, 67))}
MODES = ("roles", 1)
PAR = dict(delta=1e-9)              # (the attenuation must leave something of the stale-data test's values around 1e6: the same in every run)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _specimen(case):
    shape, planes = CASES[case]
    nz, ny, nx = shape
    rng = np.random.default_rng(81)
    v = np.zeros(shape, dtype=np.float32)
    for z in planes:
        v[z, ny // 2 - 4:ny // 2 + 4, :] = rng.random((8, nx), dtype=np.float32) + np.float32(0.25)
    return v


def _psf():
    return np.random.default_rng(82).random(PSF_SHAPE, dtype=np.float32) + 0.05


def _view(c, gt, degrees, **params):
    p = c.view_params(degrees=degrees, inc=1, snr=25.0, seed=SEED, stream=3, conv_method=1, **dict(PAR, **params))
    res = c.simulate_view(gt, _psf(), p, want=("acq",))
    q = c.queue_stats()
    res["tail"], res["planes"], res["queue"], res["path"] = c.tail_path(), c.plane_stats(), (q["bright"], q["inversion"], q["refused"]), c.extract_path()
    return res


def _run(mvs, gt, degrees, options, **params):
    with mvs.Context(0) as c:
        for k, v in options.items():
            c.set_option(k, v)
        return _view(c, gt, degrees, **params)


_REFERENCE = {}


def _reference(mvs, case, mode):
    """The 0 degree view with skip_tail = 0, default parameters: computed once, shared by the identity and the stale-data tests."""
    if (case, mode) not in _REFERENCE:
        _REFERENCE[case, mode] = _run(mvs, _specimen(case), 0, {"fused_fftx": mode, "skip_tail": 0})
    return _REFERENCE[case, mode]


def _check_identity(mvs, case, mode, degrees, extra=None, **params):
    """skip_tail = 1 against skip_tail = 0 and against skip_empty = 0 -> the skip_tail = 1 result"""
    gt, base = _specimen(case), dict(extra or {}, fused_fftx=mode)
    shared = degrees == 0 and not extra and not params
    on = _run(mvs, gt, degrees, dict(base, skip_tail=1), **params)
    off = _reference(mvs, case, mode) if shared else _run(mvs, gt, degrees, dict(base, skip_tail=0), **params)
    plain = _run(mvs, gt, degrees, dict(base, skip_empty=0), **params)
    assert on["tail"][0] == 1 and on["path"][0] == 2, (on["tail"], on["path"])        # the mode ran, in the vector sampler
    assert on["path"][2] == 16384                                                      # the full grid: a second trip
    assert off["tail"] == (0, 0) and plain["tail"] == (0, 0)
    assert on["planes"][2] > 0, on["planes"]                                           # planes were skipped
    for other in (off, plain):
        assert _same(on["acq"], other["acq"])
        assert on["corr"] == other["corr"]
        assert on["queue"] == other["queue"], (on["queue"], other["queue"])
    return on


def test_tail_walk_host_side_on_the_cpu(mvs, tmp_path):
    """tests/c_abi/tail_walk_main.cpp: the mask and walk helpers of csrc/extract_plan.h held to plain divisions, compiled by plain g++
    under ASan + UBSan (no HIP, no libmvsim.so; a child process, nothing preloaded)."""
    exe = str(tmp_path / "tail_walk_main")
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-Wextra", "-Werror", "-I" + os.path.join(os.path.dirname(os.path.abspath(mvs.__file__)), "csrc"),
           os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_abi", "tail_walk_main.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "tail walk ok:" in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]


@pytest.mark.gpu
@pytest.mark.parametrize("degrees", (0, 3))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_second_trip_keeps_every_output(mvs, case, mode, degrees):
    on = _check_identity(mvs, case, mode, degrees)
    (nz, _, _), planes = CASES[case]
    assert on["planes"][0] == nz
    if degrees == 0:       # nothing moves: exactly the specimen's planes and their neighbours are kept -- on both trips, and empty ones on both
        kept = {z + d for z in planes for d in (-1, 0, 1)}
        assert on["planes"][2] == nz - len(kept) and min(kept) < 64 <= max(kept) < nz - 1
    assert on["queue"][1] > 0                                                          # the empty planes queue their misses


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_second_trip_lets_no_stale_plane_through(mvs, case, mode):
    """After a dense view of values around 1e6 the workspace between pass E and the sampler holds that volume in every plane the sparse
    view leaves unwritten: one plane read where it must not be shows at once.  dense -> sparse -> dense -> sparse in one context, and the
    same behind a dense volume with one empty plane, as the first view of its context: the views behind it certainly carry flags (behind a
    view without empty planes the next ones may run unflagged, hence not sparse)."""
    shape = CASES[case][0]
    dense = (np.random.default_rng(83).random(shape, dtype=np.float32) + np.float32(0.5)) * np.float32(1e6)
    holed = dense.copy()
    holed[0] = 0.0
    sparse, ref = _specimen(case), _reference(mvs, case, mode)
    for big in (dense, holed):
        with mvs.Context(0) as c:
            c.set_option("fused_fftx", mode)
            first = _view(c, big, 0)
            assert float(first["acq"].max()) > 0
            second = _view(c, sparse, 0)
            assert _same(second["acq"], ref["acq"]), "dense -> sparse"
            again = _view(c, big, 0)
            assert _same(again["acq"], first["acq"]), "sparse -> dense"
            third = _view(c, sparse, 0)
            assert _same(third["acq"], ref["acq"]), "sparse -> dense -> sparse"
            if big is holed:       # flags certainly, hence the mode, planes left out, and the same items queued
                for res in (second, third):
                    assert res["tail"][0] == 1 and res["planes"][2] > 0 and res["queue"] == ref["queue"]


@pytest.mark.gpu
def test_checked_segments_on_the_second_trip(mvs):
    """poisson_queue_share = 4: segments that can fill up, the CHECKED instance"""
    on = _check_identity(mvs, "aligned", "roles", 0, extra={"poisson_queue_share": 4})
    assert on["path"][1] == 1


@pytest.mark.gpu
def test_empty_planes_in_regime_0_on_the_second_trip(mvs):
    """min_value = 0: an empty plane's one value is 0, nothing to sample there"""
    _check_identity(mvs, "aligned", "roles", 0, min_value=0.0)


@pytest.mark.gpu
def test_empty_planes_in_the_ptrs_regime_on_the_second_trip(mvs):
    """a min_value so large that the empty planes' constant is a bright voxel: the ordinary phase 1 on the constant, without a read"""
    on = _check_identity(mvs, "aligned", "roles", 0, min_value=1.0)
    assert on["queue"][0] > 0
