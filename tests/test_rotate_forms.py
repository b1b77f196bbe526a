"""Every launch form of rotate (about x) + attenuate in the per-view pipeline writes the same `rot` and `att`, and both equal the
oracle's rotateAroundAxis followed by attenuate3d bit for bit.  The forms share one statement of the arithmetic (csrc/rotate_dev.h);
they differ in who computes a row's geometry and how the loads are issued:
    fused_fftx=0 with fused_rotate=0 (separate kernels), lds (geometry table in LDS), lane (every lane recomputes it);
    fused_fftx=1 (rotate + attenuate + x transform, every wave walks and transforms), roles (walker and transformer waves).
Shapes: the smallest at which each shared helper can still go wrong (see CASES)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DELTA = 0.01
#        (nz, ny, nx)      PSF (kz, ky, kx)  degrees
CASES = [((6, 150, 130), (3, 5, 5), 33),     # Nx no multiple of 64: inactive lanes in the third wave; Ny > Nx: rows the attenuation never
                                             # visits are written to rot; partial rows at the faces; padded half length 72: both fused-FFT kernels run
         ((5, 130, 130), (3, 3, 5), 90),     # source rows exactly on the grid: zero weights, whole batches of class 1 and class 0
         ((5, 130, 130), (3, 3, 5), 0),
         ((3, 660, 640), (3, 5, 7), -40)]    # 640 steps: two 512-row geometry chunks in the LDS-table kernel, five 128-row chunks in the
                                             # 16-wave fused-FFT form (G = 2); roles falls back to the plain fused kernel
FORMS = [("0", "0"), ("0", "lds"), ("0", "lane"), ("1", None), ("roles", None)]     # (fused_fftx, fused_rotate)


@pytest.mark.parametrize("shape,kshape,degrees", CASES)
def test_every_rotate_attenuate_form_equals_the_oracle(mvs, synth, orc, shape, kshape, degrees):
    rng = np.random.default_rng(91)
    gt = synth.sphere_phantom(shape[2], shape[1], shape[0]) + (rng.random(shape, dtype=np.float32) < 0.02).astype(np.float32)
    psf = rng.random(kshape, dtype=np.float32) + 0.05
    want_rot = orc.rotate_around_axis(gt, 0, degrees)
    want_att = orc.attenuate3d(want_rot, DELTA)
    assert float(want_rot.max()) > 0 and not np.array_equal(want_att, want_rot)
    got = {}
    for fftx, rotate in FORMS:
        with mvs.Context(0) as c:
            c.set_option("fused_fftx", fftx)
            if rotate is not None:
                c.set_option("fused_rotate", rotate)
            p = c.view_params(degrees=degrees, delta=DELTA, inc=1, snr=25.0, seed=7, stream=1, conv_method=1)
            c.enable_timing(True)
            got[(fftx, rotate)] = c.simulate_view(gt, psf.copy(), p, want=("rot", "att", "acq"))
            # the fused-FFT forms really ran (the driver falls back to the other forms without a word where its geometry does not
            # allow them): they do pass A's work themselves, so the convolution has no pass A of its own
            t = c.timings()
            assert t["rotate_ms"] > 0 and (t["pass_a_ms"] == 0) == (fftx != "0"), ((fftx, rotate), t)
    for form, res in got.items():
        assert float(res["rot"].max()) > 0 and not np.array_equal(res["att"], res["rot"]), form
        for k in ("rot", "att"):
            assert np.array_equal(res[k], got[FORMS[0]][k]), (form, k)
        assert np.array_equal(res["rot"], want_rot), form
        assert np.array_equal(res["att"], want_att), form
