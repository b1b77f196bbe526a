"""The sparse tail (option skip_tail, csrc/extract_plan.h): behind a flagged view whose convolved volume nobody asked for, pass E
stores nothing into the planes whose dilated flag is clear and phase 1 of the queue samplers reads nothing there -- every voxel of such
a plane has the one value adjust_one(+0, corr, min_value).  The workspace between the two then holds stale planes of earlier views that
nothing may ever let through.  Exact: every output equals skip_tail = 0 and skip_empty = 0 bit for bit, and the same items are queued.

The cases.  The issue lists (nz, ny, nx) = (24, 64, 64), (20, 77, 70), (24, 64, 72) and (16, 512, 512), "forced onto the fused kernels
with fused_fftx".  The fused rotate kernel, the only source of plane flags, exists for padded x lengths of 144 points and more
(rot_fftx_len_ok: half lengths 72 .. 576), so no option takes rows of 64 .. 72 voxels there: such views carry no flags and can never run
the mode, and the two asserts the issue insists on (tail_path says 1, planes were skipped) cannot hold for them under any implementation.
(24, 64, 72) moreover has Nx > Ny, which the view pipeline refuses.  Each small case therefore runs at the smallest width that does reach
the fused kernel and keeps what the issue chose it for -- see CASES -- and the issue's own shapes run in
`test_shapes_below_the_fused_kernel_keep_their_stores`: identical outputs, mode 0 (the refused one: refused)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

SEED = 464232194
DEGREES = (0, 3)                    # 0: the planes beyond Kz/2 of the specimen are empty; 3 degrees keeps the slab thin

#        (nz, ny, nx)     PSF (kz, ky, kx)
CASES = [((24, 128, 128), (5, 5, 17)),         # plane of 16384 voxels = 64 slots: every slot lies in one plane (the issue's 64 x 64)
         ((20, 145, 139), (7, 5, 7)),          # plane no multiple of 4: k_extract_noise2_any (the issue's 77 x 70)
         ((24, 144, 140), (5, 5, 5)),          # 5040 groups per plane, no multiple of 64: slots straddle planes, per-lane "no read" (64 x 72)
         ((16, 512, 512), (3, 7, 31))]         # the flagship's kernel instances and line length
ISSUE_SMALL = [((24, 64, 64), (5, 5, 5)), ((20, 77, 70), (7, 5, 7))]     # below the fused kernel: no flags, no sparse tail
MODES = ("roles", 1)


def _same(a, b):
    """np.array_equal on the bit patterns (an all-zero volume has no mean to adjust to: NaN in every mode; +0 is not -0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _specimen(shape, planes=None, seed=77):
    """Random values confined to a few middle planes (or `planes`) and to the middle quarter of y, so that a small angle keeps it thin."""
    nz, ny, nx = shape
    rng = np.random.default_rng(seed)
    v = np.zeros(shape, dtype=np.float32)
    planes = range(nz // 2 - 1, nz // 2 + 1) if planes is None else planes
    y0, y1 = ny // 2 - max(1, ny // 8), ny // 2 + max(1, ny // 8)
    for z in planes:
        v[z, y0:y1, :] = rng.random((y1 - y0, nx), dtype=np.float32) + np.float32(0.25)
    return v


def _psf(kshape):
    return np.random.default_rng(78).random(kshape, dtype=np.float32) + 0.05


def _view(c, gt, psf, degrees, inc, want, **params):
    p = c.view_params(degrees=degrees, inc=inc, snr=params.pop("snr", 25.0), seed=SEED, stream=3, conv_method=1, **params)
    res = c.simulate_view(gt, psf.copy(), p, want=want)
    q = c.queue_stats()
    res["tail"], res["planes"], res["queue"] = c.tail_path(), c.plane_stats(), (q["bright"], q["inversion"], q["refused"])
    res["path"] = c.extract_path()
    return res


def _run(mvs, gt, psf, degrees, inc, options, want=("acq",), **params):
    with mvs.Context(0) as c:
        for k, v in options.items():
            c.set_option(k, v)
        return _view(c, gt, psf, degrees, inc, want, **params)


def _check_identity(mvs, gt, psf, degrees, inc, mode, expect_sparse=True, expect_skipped=True, extra=None, queued=True, **params):
    """skip_tail = 1 against skip_tail = 0 and skip_empty = 0, without and with the convolved volume; -> the skip_tail = 1 result.
    queued: the view samples through the two-launch queue, whose statistics then say which items were appended."""
    base = dict(extra or {}, fused_fftx=mode)
    on = _run(mvs, gt, psf, degrees, inc, dict(base, skip_tail=1), **params)
    off = _run(mvs, gt, psf, degrees, inc, dict(base, skip_tail=0), **params)
    plain = _run(mvs, gt, psf, degrees, inc, dict(base, skip_empty=0), **params)
    if expect_sparse is None:          # fuse_tail = 1: mode 0 iff pass E did run the fused tail (it needs rows of whole float4 groups)
        expect_sparse = on["path"][0] != 4
    assert on["tail"][0] == (1 if expect_sparse else 0), on["tail"]
    assert off["tail"] == (0, 0) and plain["tail"] == (0, 0)
    if expect_sparse:
        assert on["tail"][1] in (1, inc)
        assert (on["planes"][2] > 0) == expect_skipped, on["planes"]       # "skipped", not "would have passed anyway"
    for other in (off, plain):
        assert _same(on["acq"], other["acq"])
        assert on["corr"] == other["corr"] or (np.isnan(on["corr"]) and np.isnan(other["corr"]))
        assert not queued or on["queue"] == other["queue"], (on["queue"], other["queue"])
    # the convolved volume requested: no holes anywhere, the same volume
    con_on = _run(mvs, gt, psf, degrees, inc, dict(base, skip_tail=1), want=("con", "acq"), **params)
    con_off = _run(mvs, gt, psf, degrees, inc, dict(base, skip_tail=0), want=("con", "acq"), **params)
    assert con_on["tail"] == (0, 0)
    assert _same(con_on["con"], con_off["con"]) and _same(con_on["acq"], con_off["acq"]) and _same(con_on["acq"], on["acq"])
    return on


def test_skip_tail_host_side_on_the_cpu(mvs, tmp_path):
    """tests/c_abi/skip_tail_main.cpp: csrc/extract_plan.h compiled by plain g++ under ASan + UBSan (no HIP, no libmvsim.so; a child
    process, nothing preloaded): the host condition over all of its inputs; the flag a slot reads is the flag of the plane pass E
    skipped, strided and compact, over the (nz, inc, Kz) of the cases here and of the flagship; the slot walk against plain divisions."""
    exe = str(tmp_path / "skip_tail_main")
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-Wextra", "-Werror", "-I" + os.path.join(os.path.dirname(os.path.abspath(mvs.__file__)), "csrc"),
           os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_abi", "skip_tail_main.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "skip tail ok:" in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]


@pytest.mark.gpu
def test_shapes_below_the_fused_kernel_keep_their_stores(mvs):
    """The issue's own small shapes: rows this short never reach the fused rotate kernel, so there are no flags and the tail keeps its
    stores whatever skip_tail says; (24, 64, 72) is no view at all (Nx > Ny)."""
    for shape, kshape in ISSUE_SMALL:
        for inc in (1, 3):
            on = _check_identity(mvs, _specimen(shape), _psf(kshape), 0, inc, "roles", expect_sparse=False)
            assert on["planes"] == (0, 0, 0)
    with pytest.raises(Exception, match="Nx > Ny"):
        _run(mvs, _specimen((24, 64, 72)), _psf((5, 5, 5)), 0, 1, {"fused_fftx": "roles"})


@pytest.mark.gpu
@pytest.mark.parametrize("inc", (1, 3))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,kshape", CASES)
def test_sparse_tail_keeps_every_output(mvs, shape, kshape, mode, inc):
    """Identity, at 0 degrees and at an angle, with the default min_value (the empty planes are in the inversion regime: items are
    queued from them) and with min_value = 0 (regime 0: nothing to sample there)."""
    gt, psf = _specimen(shape), _psf(kshape)
    for degrees in DEGREES:
        on = _check_identity(mvs, gt, psf, degrees, inc, mode)
        assert on["queue"][1] > 0                                          # inversion items: the empty planes' misses among them
    _check_identity(mvs, gt, psf, DEGREES[1], inc, mode, min_value=0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,kshape", CASES)
def test_stale_planes_never_get_through(mvs, shape, kshape, mode):
    """The failure mode of the change.  The workspace between pass E and the sampler is reused from view to view: after a dense volume
    of values around 1e6 every plane the next, sparse view leaves unwritten holds that volume.  dense -> sparse -> dense -> sparse in one
    context: every sparse acquisition equals a fresh context's -- also behind a dense volume with one empty plane, after which the next
    view certainly carries flags (a view behind one without empty planes may run unflagged, hence not sparse)."""
    rng = np.random.default_rng(79)
    dense = (rng.random(shape, dtype=np.float32) + np.float32(0.5)) * np.float32(1e6)
    holed = dense.copy()
    holed[0] = 0.0
    sparse, psf = _specimen(shape), _psf(kshape)
    par = dict(delta=1e-9)             # (the attenuation must leave something of values this large)
    for inc in (1, 3):
        fresh = _run(mvs, sparse, psf, 0, inc, {"fused_fftx": mode}, **par)
        plain = _run(mvs, sparse, psf, 0, inc, {"fused_fftx": mode, "skip_tail": 0}, **par)
        assert fresh["tail"][0] == 1 and fresh["planes"][2] > 0 and _same(fresh["acq"], plain["acq"])
        for big in (dense, holed):
            with mvs.Context(0) as c:
                c.set_option("fused_fftx", mode)
                first = _view(c, big, psf, 0, inc, ("acq",), **par)
                assert float(first["acq"].max()) > 0
                second = _view(c, sparse, psf, 0, inc, ("acq",), **par)
                assert _same(second["acq"], fresh["acq"]), "dense -> sparse"
                again = _view(c, big, psf, 0, inc, ("acq",), **par)
                assert _same(again["acq"], first["acq"]), "sparse -> dense"
                third = _view(c, sparse, psf, 0, inc, ("acq",), **par)
                assert _same(third["acq"], fresh["acq"]), "sparse -> dense -> sparse"
                if big is holed:       # flags certainly, hence the mode, and planes left out
                    assert second["tail"][0] == 1 and second["planes"][2] > 0 and third["tail"][0] == 1 and third["planes"][2] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,kshape", CASES[:3])
def test_sparse_tail_edges(mvs, shape, kshape, mode):
    nz, ny, nx = shape
    psf = _psf(kshape)
    for inc in (1, 3):
        # all zero: no mean to adjust to (corr is not finite), every plane empty
        _check_identity(mvs, np.zeros(shape, dtype=np.float32), psf, 0, inc, mode)
        # a specimen at a z face: the mirrored halo makes the face planes non-empty
        _check_identity(mvs, _specimen(shape, planes=(0, 1)), psf, 0, inc, mode)
        _check_identity(mvs, _specimen(shape, planes=(nz - 1,)), psf, 0, inc, mode)
        # a single non-empty plane
        _check_identity(mvs, _specimen(shape, planes=(nz // 2,)), psf, 0, inc, mode)
        # no empty plane at all: the mode is on and skips nothing
        dense = np.random.default_rng(80).random(shape, dtype=np.float32) + np.float32(0.01)
        _check_identity(mvs, dense, psf, DEGREES[1], inc, mode, expect_skipped=False)
        # min_value so large that the empty planes' one value is in the PTRS regime: the ordinary phase 1 on the constant
        on = _check_identity(mvs, _specimen(shape), psf, 0, inc, mode, min_value=1.0)
        assert on["queue"][0] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape,kshape", CASES[:3])
def test_routes_that_keep_their_stores(mvs, shape, kshape):
    """No noise (the copy forms), the one-kernel samplers, the fused tail, stacked views: mode 0, results unchanged."""
    gt, psf = _specimen(shape), _psf(kshape)
    for inc in (1, 3):
        _check_identity(mvs, gt, psf, 0, inc, "roles", expect_sparse=False, queued=False, snr=-1.0)
        _check_identity(mvs, gt, psf, 0, inc, "roles", expect_sparse=False, queued=False, extra={"poisson_queue": 0})
        fused = _check_identity(mvs, gt, psf, 0, inc, "roles", expect_sparse=None, queued=False, extra={"fuse_tail": 1})
        assert (fused["path"][0] == 4) == (shape[2] % 4 == 0)
        stacked = {}
        for tail in (1, 0):
            with mvs.Context(0) as c:
                c.set_option("fused_fftx", "roles")
                c.set_option("skip_tail", tail)
                _view(c, gt, psf, 0, inc, ("acq",))       # a sparse view first: its holes are what a stacked view would trip over
                c.set_option("view_batch", 1)
                params = [c.view_params(degrees=d, inc=inc, snr=25.0, seed=SEED + v, stream=3, conv_method=1) for v, d in enumerate((0, 3))]
                stacked[tail] = c.simulate_views(gt, [psf.copy(), psf.copy()], params)
                assert c.tail_path() == (0, 0)
        assert _same(stacked[1][0], stacked[0][0]) and _same(stacked[1][1], stacked[0][1])
