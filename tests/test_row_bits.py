"""Row bits (csrc/row_bits.h, option skip_rows): where the plane flags are in use the fused rotate kernels do not store the rows
without a non-zero attenuated voxel, and pass B reads a per-plane bit string instead of those rows.  The workspace then holds stale
rows of earlier views that nothing may ever let through; the mirrored halo positions ask the bit of the row they mirror; a masked
row is +0.  Exact: every output equals skip_rows = 0 and the separate kernels bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

SEED = 464232194

#        (nz, ny, nx)     PSF (kz, ky, kx)  degrees
CASES = [((8, 64, 64), (5, 5, 5), 33),          # one walker wave; 72-point lines: the per-row form of pass B's bit test
         ((6, 77, 70), (5, 5, 7), -52),         # Ny > Nx: rows the attenuation never visits are zero rows
         ((5, 200, 192), (9, 9, 15), 60),       # 224-point lines: one word of the record per load iteration
         ((4, 512, 512), (3, 7, 31), 15),       # the flagship's instance and line length (560: two words per iteration)
         ((4, 512, 512), (3, 7, 31), 90),
         ((3, 600, 576), (3, 5, 9), 25),        # nine waves: the kernel every wave walks and transforms in; 8-column tiles
         # 0 degrees: the rotated rows ARE the input's, so the single-voxel volumes below store exactly row 0 / row Ny - 1 (under the
         # angles above a voxel of an outer row of these thin volumes leaves the volume: a legitimate all-zero view)
         ((8, 64, 64), (5, 5, 5), 0),
         ((6, 77, 70), (5, 5, 7), 0),
         ((4, 512, 512), (3, 7, 31), 0),
         ((3, 600, 576), (3, 5, 9), 0)]
VOLUMES = ("phantom", "dense", "zero", "voxel_y0", "voxel_ylast", "band")


def _same(a, b):
    """np.array_equal on the bit patterns: an all-zero volume has no mean to adjust to, its `con` is NaN in every mode; and +0 is
    not -0 here."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _volume(synth, kind, shape):
    nz, ny, nx = shape
    rng = np.random.default_rng(77)
    if kind == "phantom":
        return synth.sphere_phantom(nx, ny, nz) + (rng.random(shape, dtype=np.float32) < 0.02).astype(np.float32)
    if kind == "dense":
        return rng.random(shape, dtype=np.float32) + np.float32(0.01)
    v = np.zeros(shape, dtype=np.float32)
    if kind == "voxel_y0":          # one stored row beside unstored ones, mirrored by the halo at the end of the padded line
        v[nz // 2, 0, nx // 3] = 1.0
    elif kind == "voxel_ylast":     # ... and by the halo right of the data rows
        v[nz // 2, ny - 1, nx // 3] = 1.0
    elif kind == "band":            # a specimen confined to four rows
        v[:, ny // 2:ny // 2 + 4, :] = rng.random((nz, 4, nx), dtype=np.float32) + np.float32(0.5)
    return v


def _psf(kshape):
    return np.random.default_rng(78).random(kshape, dtype=np.float32) + 0.05


def _run(mvs, gt, psf, degrees, options, wants=(("rot", "att", "con", "acq"), ("acq",)), **params):
    with mvs.Context(0) as c:
        for k, v in options.items():
            c.set_option(k, v)
        p = c.view_params(degrees=degrees, inc=1, snr=25.0, seed=SEED, stream=3, conv_method=1, **params)
        return [c.simulate_view(gt, psf.copy(), p, want=w) for w in wants]


def test_row_bit_record_on_the_cpu(mvs, tmp_path):
    """tests/c_abi/row_bits_main.cpp: csrc/row_bits.h compiled by plain g++ under ASan + UBSan (no HIP, no libmvsim.so; a child
    process, nothing preloaded).  Every (Ny, Ky, Py) of the length table for Ny in {1, 2, 5, 64, 77, 289, 512, 1024} and Ky in
    {1, 3, 9, 31, 63}, eight stored-row sets each: the padded record equals its restatement through map_src bit by bit, gap bits are
    clear, sizes and alignment are what the driver allocates."""
    exe = str(tmp_path / "row_bits_main")
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-Wextra", "-Werror", "-I" + os.path.join(os.path.dirname(os.path.abspath(mvs.__file__)), "csrc"),
           os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_abi", "row_bits_main.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "row bits ok: 320 cases" in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]


@pytest.mark.gpu
@pytest.mark.parametrize("volume", VOLUMES)
@pytest.mark.parametrize("shape,kshape,degrees", CASES)
def test_row_bits_keep_every_output(mvs, synth, shape, kshape, degrees, volume):
    """Identity: skip_rows = 1 against skip_rows = 0 under both fused kernels, and against the separate kernels."""
    gt, psf = _volume(synth, volume, shape), _psf(kshape)
    ref = _run(mvs, gt, psf, degrees, {"fused_fftx": 0})
    for mode in ("roles", 1):
        for rows in (1, 0):
            got = _run(mvs, gt, psf, degrees, {"fused_fftx": mode, "skip_rows": rows})
            for k in ("rot", "att", "con", "acq"):
                assert _same(got[0][k], ref[0][k]), (k, mode, rows)
            assert _same(got[1]["acq"], ref[1]["acq"]), (mode, rows)
    att = ref[0]["att"]
    nz, ny, nx = shape
    if volume == "zero":
        assert not att.any()
    elif volume in ("phantom", "dense", "band"):
        assert float(att.max()) > 0
    elif degrees == 0 and (volume == "voxel_ylast" or ny <= nx):    # (Ny > Nx: the attenuation never visits row 0)
        y = ny - 1 if volume == "voxel_ylast" else 0
        assert float(att[nz // 2, y].max()) > 0 and np.count_nonzero(att.reshape(nz * ny, nx).any(axis=1)) == 1   # ONE stored row


@pytest.mark.gpu
@pytest.mark.parametrize("shape,kshape,degrees", [CASES[0], CASES[1], CASES[3], CASES[6], CASES[8]])   # (0 degrees: an empty plane stays empty)
@pytest.mark.parametrize("mode", ("roles", 1))
def test_stale_workspace_rows_never_get_through(mvs, synth, shape, kshape, degrees, mode):
    """The workspace is reused from view to view: after a dense volume of large values every row the next, sparse view leaves
    unwritten holds that volume's spectrum.  The sparse view must come out as from a fresh context, bit for bit -- in the orders
    dense -> sparse and sparse -> dense -> sparse, and with a dense volume that keeps one plane empty, after which the next view
    certainly carries flags and row bits (a view behind one without empty planes may run unflagged)."""
    nz, ny, nx = shape
    rng = np.random.default_rng(79)
    dense = (rng.random(shape, dtype=np.float32) + np.float32(0.5)) * np.float32(1e6)
    holed = dense.copy()
    holed[0] = 0.0
    psf = _psf(kshape)
    opts = {"fused_fftx": mode}
    par = dict(delta=1e-9)         # (the attenuation must leave something of values this large)
    for kind in ("voxel_y0", "voxel_ylast", "band"):
        sparse = _volume(synth, kind, shape)
        fresh = _run(mvs, sparse, psf, degrees, opts, wants=(("acq", "con"),), **par)[0]
        plain = _run(mvs, sparse, psf, degrees, {"fused_fftx": mode, "skip_rows": 0}, wants=(("acq", "con"),), **par)[0]
        assert _same(fresh["acq"], plain["acq"]) and _same(fresh["con"], plain["con"]), kind
        for big in (dense, holed):
            with mvs.Context(0) as c:
                c.set_option("fused_fftx", mode)
                p = c.view_params(degrees=degrees, inc=1, snr=25.0, seed=SEED, stream=3, conv_method=1, **par)
                first = c.simulate_view(big, psf.copy(), p, want=("acq", "con"))
                assert np.isfinite(first["con"]).all() and float(first["con"].max()) > 0
                second = c.simulate_view(sparse, psf.copy(), p, want=("acq", "con"))
                assert _same(second["acq"], fresh["acq"]) and _same(second["con"], fresh["con"]), (kind, "dense -> sparse")
                again = c.simulate_view(big, psf.copy(), p, want=("acq", "con"))
                assert _same(again["acq"], first["acq"]) and _same(again["con"], first["con"]), (kind, "sparse -> dense")
                third = c.simulate_view(sparse, psf.copy(), p, want=("acq", "con"))
                assert _same(third["acq"], fresh["acq"]) and _same(third["con"], fresh["con"]), (kind, "sparse -> dense -> sparse")


@pytest.mark.gpu
@pytest.mark.parametrize("volume", ("phantom", "voxel_y0", "band"))
def test_configurations_without_row_bits_keep_working(mvs, synth, volume):
    """skip_empty = 0 (no flags, hence no record), a z slab of a tiled view and two stacked views keep the zero stores: skip_rows = 1
    gives what skip_rows = 0 gives."""
    shape, kshape, degrees = CASES[0]
    nz, ny, nx = shape
    gt, psf = _volume(synth, volume, shape), _psf(kshape)
    a = _run(mvs, gt, psf, degrees, {"fused_fftx": "roles", "skip_empty": 0, "skip_rows": 1})
    b = _run(mvs, gt, psf, degrees, {"fused_fftx": "roles", "skip_empty": 0, "skip_rows": 0})
    for k in ("rot", "att", "con", "acq"):
        assert _same(a[0][k], b[0][k]), k
    assert _same(a[1]["acq"], b[1]["acq"])
    slabs, stacked = {}, {}
    for rows in (1, 0):
        with mvs.Context(0) as c:
            c.set_option("fused_fftx", "roles")
            c.set_option("skip_rows", rows)
            d_gt, d_acq = c.dev_alloc(gt.nbytes), [c.dev_alloc(gt.nbytes) for _ in range(2)]
            try:
                c.upload(d_gt, gt)
                # a whole view first: its unwritten rows are what a slab's or a stacked view's pass B would trip over
                p = c.view_params(degrees=degrees, inc=1, snr=25.0, seed=SEED, stream=3, conv_method=1)
                c.simulate_view_dev(d_gt, (nx, ny, nz), psf.copy(), p, d_acq[0])
                k = c.view_slab_dev(d_gt, (nx, ny, nz), psf.copy(), p, 2, 6, d_acq[0])
                c.synchronize()
                assert k == 4
                slabs[rows] = c.download(d_acq[0], (k, ny, nx))
                c.set_option("view_batch", 1)
                params = [c.view_params(degrees=d, inc=1, snr=25.0, seed=SEED + v, stream=3, conv_method=1) for v, d in enumerate((degrees, -degrees))]
                c.simulate_views_dev(d_gt, (nx, ny, nz), [psf.copy(), psf.copy()], params, d_acq)
                c.synchronize()
                stacked[rows] = [c.download(x, shape) for x in d_acq]
            finally:
                for x in [d_gt] + d_acq:
                    c.dev_free(x)
    assert _same(slabs[1], slabs[0])
    assert _same(stacked[1][0], stacked[0][0]) and _same(stacked[1][1], stacked[0][1])
